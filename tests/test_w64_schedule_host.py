"""The case table of tests/w64_schedule.py has no holes, proven without a GPU: every template form of k_grad_w64 gets a workgroup
in every cell of the row walk, every tabulated seed keeps the problem off the ReLU kink, and a walk that drops a block, counts
one twice or counts the ragged block's padding misses the per-leaf bound of tests/test_gpu_w64_schedule.py by more than 10x
(measured on the fp64 oracle: 290x at the least, the one-row last block of N = 225; 340x for the padding, N = 351)."""
import numpy as np
import pytest

from tests import leafcheck as L
from tests import w64_schedule as W

FORM_IDS = [W.form_id(f) for f in W.FORMS]
NET_IDS = [f'NH{len(hs) - 1}-F{F}' for F, hs in W.NETS]


# ---- the restatement and the table --------------------------------------------------------------------------------------------

def test_restated_schedule_on_known_launches():
    """w64_S and the b0 / b1 formula on the launches tests/test_gpu_parity.py records (LAUNCH_SHAPES: grid (8, 16) for N = 1052,
    E = 16) and on the benchmark's B2 net (128 particles of 1052 rows: two workgroups of 16 and 17 blocks)."""
    assert W.splits(1052, 16) == 8 and W.blocks(1052, 8) == [4, 4, 4, 4, 4, 4, 4, 5]
    assert W.splits(1052, 128) == 2 and W.blocks(1052, 2) == [16, 17]
    assert W.splits(33, 300) == 1 and W.blocks(33, 1) == [2]
    assert W.splits(2, 1) == 1 and W.blocks(2, 1) == [1]
    assert W.splits(4096, 1, n_cu=304) == 32                                   # NB / 4 binds before the CU count
    for rows, S in ((1052, 8), (301, 2), (7, 2), (855, 4)):
        b, b0 = W.blocks(rows, S), W.first_blocks(rows, S)
        assert sum(b) == (rows + 31) // 32 and b0 == [sum(b[:s]) for s in range(S)]
    assert [W.cell(n) for n in (0, 1, 3, 4, 7, 8, 10, 15, 40)] == [(0, 0), (0, 1), (0, 3), (1, 0), (1, 3), (2, 0), (2, 2), (2, 3), (2, 0)]
    assert len(W.CELLS) == 12 and len(W.NONEMPTY_CELLS) == 11


def test_the_ten_forms():
    assert len(W.FORMS) == len(set(W.FORMS)) == 10 and len(W.NETS) == 6
    seen = set()
    for F, hs, k in W.FORMS:
        nh, fq = len(hs) - 1, (F + 7) // 8
        assert hs == (64,) * nh + (2,) and nh in (1, 2, 3) and fq in (1, 2) and 1 <= F <= 16
        assert k == 'mfma_w64' or (k == 'mfma_w64_bf16x3' and nh >= 2)
        seen.add((nh, fq, k))
    assert len(seen) == 10
    assert {F for F, hs, _ in W.FORMS if len(hs) == 4} == {5, 16} and {F for F, hs, _ in W.FORMS if len(hs) < 4} == {5, 12}


def test_tables_state_what_the_formula_gives():
    for (N, E), want in W.FULL_BLOCKS.items():
        assert W.blocks(N, W.splits(N, E)) == want, (N, E)
    S = W.splits(W.WINDOW_N, W.WINDOW_E)
    assert S == 2
    for (begin, count), want in W.WINDOW_BLOCKS.items():
        assert W.blocks(count, S) == want, (begin, count)
        assert begin % 32 and 0 < count and begin + count <= W.WINDOW_N
    assert any(b + c == W.WINDOW_N for b, c in W.WINDOW_CASES)                  # one window ends at the last row
    # what the issue's table names, still there
    for k in range(1, 8):
        assert (32 * k - 5, 2) in W.FULL_BLOCKS
    for k in (8, 9, 11, 12):
        assert W.FULL_BLOCKS[(32 * k - 5, 130)] == [k]
    for case in ((251, 2), (283, 2), (351, 128), (416, 128), (477, 128), (571, 64), (855, 64), (97, 2), (225, 2)):
        assert case in W.FULL_BLOCKS
    assert set(W.WINDOW_CASES) == {(13, 32), (13, 96), (13, 160), (13, 224), (13, 288), (45, 7)}


@pytest.mark.parametrize('form', W.FORMS, ids=FORM_IDS)
def test_full_cases_reach_every_cell(form):
    """Every form runs every case, so every form gets all 11 non-empty cells; each cell also on its own in a one-workgroup
    launch, where a failure can only be that cell's."""
    reached, alone = set(), set()
    for case in W.FULL_CASES:
        b = W.blocks(case[0], W.splits(*case))
        assert all(n > 0 for n in b), case                   # the empty workgroup is the windows' alone
        reached |= {W.cell(n) for n in b}
        if len(b) == 1:
            alone.add(W.cell(b[0]))
    assert reached == set(W.NONEMPTY_CELLS) and alone == set(W.NONEMPTY_CELLS), form


def test_ragged_block_visits_every_path():
    """N = 32 k - 5: the 27-row block is the last of the last workgroup -- main-loop wave 3 (rem 0), pair 0 (rem 1), pair 1 (rem 2),
    wave 2 of the three-block round (rem 3), behind 0, 1 and 2 rounds.  One valid row: main loop (97, and 225 in the second
    workgroup) and the three-block round behind a full round (193).  One case fills its last block."""
    ragged = {W.cell(W.FULL_BLOCKS[c][-1]) for c in W.FULL_CASES if c[0] % 32 == 27}
    assert ragged == set(W.NONEMPTY_CELLS)
    assert W.cell(W.FULL_BLOCKS[(97, 2)][-1]) == (1, 0) and 97 % 32 == 1
    assert W.cell(W.FULL_BLOCKS[(225, 2)][-1]) == (1, 0) and 225 % 32 == 1 and len(W.FULL_BLOCKS[(225, 2)]) == 2
    assert W.cell(W.FULL_BLOCKS[(193, 2)][-1]) == (1, 3) and 193 % 32 == 1
    assert [c for c in W.FULL_CASES if c[0] % 32 == 0] == [(416, 128)]


def test_window_cases_add_the_empty_workgroup_and_every_tail_off_block_zero():
    S = W.splits(W.WINDOW_N, W.WINDOW_E)
    cells, rems = set(), set()
    for begin, count in W.WINDOW_CASES:
        for n, b0 in zip(W.blocks(count, S), W.first_blocks(count, S)):
            cells.add(W.cell(n))
            if b0 != 0:
                rems.add(n & 3)
    assert (0, 0) in cells and rems == {0, 1, 2, 3}
    assert (0, 0) not in {W.cell(n) for c in W.FULL_CASES for n in W.FULL_BLOCKS[c]}


# ---- seeds --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('net', W.NETS, ids=NET_IDS)
def test_tabulated_seeds_keep_every_row_off_the_kink(net):
    """No row is masked (that would move a case into another cell): the tabulated seed is the first in 0..9 with no hidden
    pre-activation within 3e-7 of its layer's largest, on the fp64 oracle.  The windows are rows of the N = 301 problem, whose
    layer maxima bound theirs."""
    form = net + ('mfma_w64',)
    for N in sorted({N for N, _ in W.FULL_CASES} | {W.WINDOW_N}):
        seed = W.seed_of(form, N)
        assert 0 <= seed < W.SEED_TRIES
        assert W.near_kink(net, N, seed) == 0, (net, N, seed)
        assert seed == W.first_clean_seed(net, N), (net, N, seed)
    assert all((F, nh) in {(n[0], len(n[1]) - 1) for n in W.NETS} and N in {c[0] for c in W.FULL_CASES} for F, nh, N in W.SEEDS)


def test_problem_tiles_two_chains():
    form = W.FORMS[-1]
    ospec, X, y, theta = W.problem(form, 59, 5, 0)
    assert X.shape == (59, form[0]) and y.shape == (59,) and theta.shape == (5, ospec.n_params) and theta.dtype == np.float32
    assert np.array_equal(theta[2], theta[0]) and np.array_equal(theta[4], theta[0]) and np.array_equal(theta[3], theta[1])
    assert not np.array_equal(theta[0], theta[1])
    _, X2, _, th2 = W.problem(form, 59, 130, 0)
    assert np.array_equal(X2, X) and np.array_equal(th2[:5], theta)       # the data and the two chains do not depend on E
    lp, g, g32 = W.reference((form[0], form[1]), 59, 0)
    assert lp.shape == (2,) and g.shape == (2, ospec.n_params) and g32.dtype == np.float32
    lpw, gw, _ = W.reference((form[0], form[1]), 59, 0, 13, 32)
    assert np.abs(gw - g).max() > 0


# ---- mutants ------------------------------------------------------------------------------------------------------------------

def _patterns():
    seen, out = set(), []
    for case in W.FULL_CASES:
        key = (tuple(W.FULL_BLOCKS[case]), case[0] % 32)
        if key not in seen:
            seen.add(key)
            out.append(case)
    return out


@pytest.mark.parametrize('net', W.NETS, ids=NET_IDS)
def test_a_walk_that_is_one_block_off_misses_the_bound_tenfold(net):
    """For every distinct block pattern: the gradient with a block dropped, a block counted twice (the first block of the first
    workgroup; the last of the last, which is the ragged one) and the ragged block's padded rows counted as copies of row N - 1,
    built from row subsets of the fp64 oracle with the prior counted once.  Each misses the GPU test's per-leaf bound -- 5e-5, or
    8x the float32 oracle's own error -- on some leaf by 10x or more, and the float32 oracle itself is inside it.  The split and
    fp32 kernel forms of a net share its oracle, so the six nets stand for the ten forms."""
    ospec = W.ospec_of(net)
    leaves = L.fcn_leaves(ospec)
    form = net + ('mfma_w64',)
    for N, E in _patterns():
        seed = W.seed_of(form, N)
        _, g, g32 = W.reference(net, N, seed)
        bound = L.leaf_bounds(leaves, 2, g32=g32, g_ref=g, tol=L.LEAF_TOL, margin=L.F32_MARGIN)
        L.assert_leaves(g32, g, leaves, bound, tag=(net, N, 'float32 oracle'))
        mutants = W.schedule_mutants(N, W.splits(N, E))
        assert len(mutants) == (5 if N % 32 else 4)
        for name, rows in mutants.items():
            g_mut = W.gradient_over(net, N, seed, rows)
            ratio = (L.leaf_errors(g_mut, g, leaves) / bound).max(axis=1)
            assert ratio.min() >= 10.0, (net, N, E, name, ratio)                 # in both chains
            with pytest.raises(AssertionError, match='leaf'):
                L.assert_leaves(g_mut, g, leaves, bound, tag=name)
        whole = W.gradient_over(net, N, seed, np.arange(N))
        assert np.array_equal(whole, g)                                          # the row-subset path is the reference's

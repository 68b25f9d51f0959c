"""How k_grad_w64 walks the row blocks, restated, and the cases that put a workgroup into every cell of that walk (no torch, no
GPU; tests/test_w64_schedule_host.py proves the table on the CPU, tests/test_gpu_w64_schedule.py runs it).

The kernel (mile_amd/csrc/mile_grad_w64.h): workgroup s of S owns the 32-row blocks [s NB / S, (s + 1) NB / S) of NB = Npad / 32
(the window's own padded count under a row window, with S still taken from the full set: w64_S in mile_hip.hip).  With nblk
blocks it runs nblk >> 2 rounds of one block per wave (X prefetched one round ahead), then a tail for rem = nblk & 3: three
independent waves (rem 3), wave pairs sharing a block (rem 1, 2; the idle pair only counts barriers), or nothing.  A cell is
(min(rounds, 2), rem): 12 of them, (0, 0) being the workgroup without a block that only a window produces.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

N_CU = 256                      # an MI355X


# ---- the schedule -------------------------------------------------------------------------------------------------------------

def splits(N_full, E, n_cu=N_CU):
    """w64_S: workgroups per particle, from the full data set's block count whatever the window."""
    NB = (int(N_full) + 31) // 32
    return min(max(1, n_cu // max(int(E), 1)), max(1, NB // 4))


def blocks(rows, S):
    """nblk of every workgroup for `rows` rows (the full set's, or a window's count)."""
    NB = (int(rows) + 31) // 32
    return [(s + 1) * NB // S - s * NB // S for s in range(S)]


def first_blocks(rows, S):
    """b0 of every workgroup."""
    NB = (int(rows) + 31) // 32
    return [s * NB // S for s in range(S)]


def cell(nblk):
    """(main-loop rounds capped at 2, leftover blocks)."""
    return (min(nblk >> 2, 2), nblk & 3)


CELLS = [(r, m) for r in range(3) for m in range(4)]
NONEMPTY_CELLS = [c for c in CELLS if c != (0, 0)]


# ---- the kernel's template forms ----------------------------------------------------------------------------------------------

def _hidden(nh):
    return (64,) * nh + (2,)


# (F, hidden, kernel): NH in {1, 2, 3} hidden layers, FQ = 1 (F <= 8) or 2 (F 9..16), fp32 MFMA or (NH >= 2) split bf16
FORMS = [(F, _hidden(nh), k)
         for nh, Fs in ((1, (5, 12)), (2, (5, 12)), (3, (5, 16)))
         for F in Fs
         for k in (('mfma_w64',) if nh == 1 else ('mfma_w64', 'mfma_w64_bf16x3'))]
NETS = sorted({(F, hs) for F, hs, _ in FORMS}, key=lambda n: (len(n[1]), n[0]))      # what the fp64 oracle distinguishes


def form_id(form):
    F, hs, k = form
    return f'NH{len(hs) - 1}-F{F}-{"split" if k == "mfma_w64_bf16x3" else "fp32"}'


def fp32_form(form):
    return (form[0], form[1], 'mfma_w64')


# ---- the cases ----------------------------------------------------------------------------------------------------------------

# (N, E) -> nblk of every workgroup at 256 CUs.  N = 32 k - 5 keeps the ragged block (27 valid rows) the last block of the last
# workgroup, so it visits main-loop wave 3, pair 0, pair 1 and wave 2 of the three-block round in turn.
FULL_BLOCKS = {}
for _k in range(1, 8):
    FULL_BLOCKS[(32 * _k - 5, 2)] = [_k]                    # one workgroup, 1..7 blocks
FULL_BLOCKS[(251, 2)] = [4, 4]
FULL_BLOCKS[(283, 2)] = [4, 5]
for _k in (8, 9, 10, 11, 12):
    FULL_BLOCKS[(32 * _k - 5, 130)] = [_k]                  # more particles than half the CUs: one workgroup, two and three rounds
FULL_BLOCKS[(351, 128)] = [5, 6]
FULL_BLOCKS[(416, 128)] = [6, 7]                            # no ragged block
FULL_BLOCKS[(477, 128)] = [7, 8]
FULL_BLOCKS[(571, 64)] = [4, 5, 4, 5]
FULL_BLOCKS[(855, 64)] = [6, 7, 7, 7]
# one valid row in the last block: in main-loop wave 3 of the only workgroup (97), of the second workgroup (225: eight blocks,
# [4, 4]) and in wave 0 of the three-block round behind a full round (193)
FULL_BLOCKS[(97, 2)] = [4]
FULL_BLOCKS[(225, 2)] = [4, 4]
FULL_BLOCKS[(193, 2)] = [7]
FULL_CASES = list(FULL_BLOCKS)

# N = 301, E = 2: S = 2.  (begin, count) -> nblk of the two workgroups; begins are not 32-aligned, (13, 288) ends at the last row
WINDOW_N, WINDOW_E = 301, 2
WINDOW_BLOCKS = {(13, 32): [0, 1], (13, 96): [1, 2], (13, 160): [2, 3], (13, 224): [3, 4], (13, 288): [4, 5], (45, 7): [0, 1]}
WINDOW_CASES = list(WINDOW_BLOCKS)


def case_id(case):
    return f'N{case[0]}-E{case[1]}'


def window_id(win):
    return f'rows{win[0]}+{win[1]}'


# ---- problems -----------------------------------------------------------------------------------------------------------------

KINK = 3e-7                     # of the layer's largest |z|: tests/test_gpu_parity.py's figure for "within fp32 rounding of the kink"
SEED_TRIES = 10
# The first seed in 0..9 whose two-chain problem has no hidden pre-activation within KINK of zero, judged on the fp64 oracle
# (first_clean_seed; tests/test_w64_schedule_host.py checks every entry).  Seed 0 wherever nothing is listed.
SEEDS = {
    # (F, hidden layers, N): seed
    (5, 1, 477): 1, (12, 2, 283): 1, (12, 2, 855): 1, (16, 3, 219): 1, (16, 3, 251): 1,
}


def ospec_of(net):
    from oracle import mclmc_oracle as M
    return M.ModelSpec(net[0], tuple(net[1]))


def draw(net, N, seed):
    """oracle.synthetic_problem at two chains."""
    from oracle import mclmc_oracle as M
    return M.synthetic_problem(ospec_of(net), N, 2, seed=seed)


def near_kink(net, N, seed):
    """Number of hidden pre-activations of the two-chain problem within KINK of their layer's largest, all hidden layers at once."""
    from oracle import mclmc_oracle as M
    prob = draw(net, N, seed)
    _, zs, _ = M.mlp_forward(ospec_of(net), prob['theta0'].astype(np.float64), prob['X'], keep=True)
    return int(sum((np.abs(z) < KINK * np.abs(z).max()).sum() for z in zs[:-1]))


def first_clean_seed(net, N):
    for seed in range(SEED_TRIES):
        if near_kink(net, N, seed) == 0:
            return seed
    raise AssertionError(f'no seed in 0..{SEED_TRIES - 1} keeps every pre-activation of {net}, N = {N} off the ReLU kink')


def seed_of(form, N):
    return SEEDS.get((form[0], len(form[1]) - 1, N), 0)


def problem(form, N, E, seed):
    """(ospec, X, y, theta [E, d]): the two-chain problem of `seed`, its two parameter rows tiled to E particles (particle e is
    chain e % 2), so the fp64 reference stays at two rows and the kink condition does not depend on E."""
    prob = draw((form[0], form[1]), N, seed)
    theta = np.ascontiguousarray(np.tile(prob['theta0'], ((E + 1) // 2, 1))[:E])
    return ospec_of((form[0], form[1])), prob['X'], prob['y'], theta


@lru_cache(maxsize=None)
def reference(net, N, seed, begin=0, count=0):
    """(logp [2], g [2, d]) in fp64 and the gradient of the same oracle evaluated at float32, on rows [begin, begin + count) (count
    0: all rows).  Shared between tests: treat as read-only."""
    from oracle import mclmc_oracle as M
    ospec, prob = ospec_of(net), draw(net, N, seed)
    sl = slice(begin, begin + count) if count else slice(None)
    X, y = prob['X'][sl], prob['y'][sl]
    lp, g = M.logpost_and_grad(ospec, prob['theta0'].astype(np.float64), X, y)
    _, g32 = M.logpost_and_grad(ospec, prob['theta0'], X, y)
    assert g.dtype == np.float64 and g32.dtype == np.float32
    for a in (lp, g, g32):
        a.setflags(write=False)
    return lp, g, g32


def gradient_over(net, N, seed, rows):
    """The fp64 oracle's gradient over the rows `rows` (an index array, repeats allowed), the prior counted once."""
    from oracle import mclmc_oracle as M
    ospec, prob = ospec_of(net), draw(net, N, seed)
    rows = np.asarray(rows, dtype=np.int64)
    return M.logpost_and_grad(ospec, prob['theta0'].astype(np.float64), prob['X'][rows], prob['y'][rows])[1]


def block_rows(N, b):
    """Valid rows of 32-row block b."""
    return np.arange(32 * b, min(32 * b + 32, N))


def schedule_mutants(N, S):
    """{name: row index array} of what a wrong walk would sum: a block dropped (a) or counted twice (b) -- the first block of the
    first workgroup and the last block of the last (the ragged one, the fewest rows) -- and the ragged block's padded rows counted
    as copies of row N - 1 (c; none when N fills its last block)."""
    NB = (N + 31) // 32
    rows = np.arange(N)
    out = {}
    for tag, b in (('first', first_blocks(N, S)[0]), ('last', NB - 1)):
        blk = block_rows(N, b)
        out[f'dropped-{tag}'] = np.setdiff1d(rows, blk)
        out[f'twice-{tag}'] = np.concatenate([rows, blk])
    if N % 32:
        out['padding-counted'] = np.concatenate([rows, np.full(32 * NB - N, N - 1)])
    return out

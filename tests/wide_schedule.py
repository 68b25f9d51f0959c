"""What launch_grad_wide<TERMS> and launch_mm3_k decide, restated, and the cases that put a launch into every cell of that
schedule (no torch, no GPU; tests/test_wide_schedule_host.py proves the table on the CPU, tests/test_gpu_wide_schedule.py runs it).

The path (mile_amd/csrc/mile_hip.hip: launch_grad_wide and, for each product, layer_fwd / layer_dw / layer_dh over the LayerPlan of
mile_amd/csrc/mile_layer_plan.h; mile_amd/csrc/mile_mm3.h): the rows -- the data set's, or a row window's -- are walked in chunks
of R rows, R fixed when launch_grad_wide lays out the activation workspace.  Per chunk: one forward k_mm3 per layer (layer_fwd),
the head -- k_wide_headblock<K, WFULL> + k_wide_headblock_reduce where the three-term form has at least two layers, a last hidden
width <= 256 and <= WH_KMAX outputs (`headblock` in launch_grad_wide), else k_wide_head on the outputs of a K-wide forward GEMM --
and per layer, top down, a dW k_mm3 with the bias column sums (layer_dw) and a dH k_mm3 (layer_dh).  launch_mm3_k picks the
predicate-free FULL instantiation, 16-byte or scalar C access and the XCD placement; k_mm3 itself walks K in chunks of 32
(mile_mm3.h:484) of one or two 16-wide k-steps (508).

CELLS are projections of a launch, not the Cartesian product of its properties.  The pruning rule: a property is crossed with
another one only where one piece of code reads both.  The row predicates (M), the column predicates (N) and the K walk of k_mm3 are
separate code, so each is crossed with the product form alone; the epilogue reads the activation, FULL, ACCUM and c_vec together
with the form, so (form, activation, FULL), (dW: accumulate, FULL) and (dW: c_vec and why, accumulate) are cells; the XCD
placement is index arithmetic ahead of everything, crossed with the form, FULL (whose loads trust the tile index) and, for
placement 1, whether M tiles remain beyond the last group of eight.  The column sums are crossed with the M tile count (only M
tile 0 may write them) and accumulate.  The head block is K x WFULL (the template), and (blocks, rows of the last block,
accumulate) pairwise; the fallback head (reason, task); the walk by chunk pattern, window kind, a window longer than a chunk and
the `mixed` memset.  The one-term form shares k_mm3's tiling and predicates: it gets the (form, FULL) cells on ReLU, and the
chunked dW.  Outputs stay <= 16 (fwd-noact and the K-wide products are then always one ragged N tile).
"""
from __future__ import annotations

from collections import namedtuple
from functools import lru_cache

import numpy as np

# ---- constants of the code (tests/test_wide_schedule_host.py parses them out of the sources) -------------------------------------
TILE = 128                      # C tile of k_mm3, both ways (launch_mm3_k: p.M % 128, (p.N + 127) / 128)
KC = 32                         # MILE_MM_KC
KSTEP = 16                      # k-step of the bf16 MFMA (mile_mm3.h:508)
HB_ROWS = 512                   # rows per workgroup of k_wide_headblock (launch_grad_wide)
HB_WAVES = 4                    # a wave takes every fourth row of its block (mile_mm3.h:670)
WH_KMAX = 8
WS_GB = 16.0                    # MILE_WIDE_WS_GB default (launch_grad_wide)
X3, X1, GEMM = 'mfma_wide_bf16x3', 'mfma_wide_bf16', 'gemm_f32'

Case = namedtuple('Case', 'name F hidden act task prior N E chunk_rows window kernel')


def _c(name, F, hidden, act, task, N, E=2, prior='Normal', chunk_rows=None, window=None, kernel=X3):
    return Case(name, F, tuple(hidden), act, task, prior, N, E, chunk_rows, window, kernel)


def up8(v):
    return (v + 7) // 8 * 8


# ---- the schedule ------------------------------------------------------------------------------------------------------------------

def offsets(case):
    """(b_off, w_off, d, dp): bias then kernel per layer (layout_fcn), slab rows padded to 4 floats (launch_grad)."""
    off, b_off, w_off, fin = 0, [], [], case.F
    for w in case.hidden:
        b_off.append(off)
        off += w
        w_off.append(off)
        off += fin * w
        fin = w
    return b_off, w_off, off, (off + 3) // 4 * 4


def layout_rows(hidden, E, N_full, chunk_rows=None):
    """R of the workspace layout (launch_grad_wide, on LayerPlan::per_row floats per row): what 16 GiB hold, at least 128, whole
    128s when below the data set, MILE_GEMM_ROWS over it all.  N_full is the data set's row count when the layout is made,
    whatever the window."""
    wp = [up8(w) for w in hidden]
    per_row = sum(wp) + 2 * max(wp)
    budget = int(WS_GB * float(1 << 30) / 4.0)
    R = budget // (E * per_row)
    R = min(max(R, 128), N_full)
    if R < N_full:
        R = max(128, R // 128 * 128)
    if chunk_rows is not None:
        R = max(1, min(int(chunk_rows), N_full))
    return R


def mm3(form, act, M, N, K, ldc, sC, c_off, accumulate, colsum, E, terms, chunk, layer):
    """launch_mm3_k (mile_hip.hip) on one product; c_off is C's offset in floats from a 256-byte aligned allocation."""
    nx, ny = (N + TILE - 1) // TILE, (M + TILE - 1) // TILE
    c_vec = ldc % 4 == 0 and sC % 4 == 0 and (4 * c_off) % 16 == 0                         # q.c_vec
    xcd = 2 if (colsum and E % 8 == 0) else (1 if (not colsum and nx > 1 and ny >= 8) else 0)   # q.xcd_remap
    nk = (K + KC - 1) // KC                                                               # mile_mm3.h:484
    last = K - KC * (nk - 1)
    return dict(kind='mm3', form=form, act=act, M=M, N=N, K=K, FULL=M % TILE == 0 and N % TILE == 0, ldc=ldc, sC=sC, c_off=c_off,
                c_vec=bool(c_vec), why=('vec' if c_vec else ('ldc' if ldc % 4 else 'base')), xcd=xcd, nx=nx, ny=ny, grid=(nx, ny, E),
                accumulate=bool(accumulate), colsum=bool(colsum), nk=nk, last=last,
                last_ksteps=min(KC // KSTEP, (last + KSTEP - 1) // KSTEP),                 # mile_mm3.h:508
                terms=terms, chunk=chunk, layer=layer)


def headblock_of(case, terms):
    hs = case.hidden
    return terms == 3 and len(hs) >= 2 and hs[-2] <= 256 and hs[-1] <= WH_KMAX             # launch_grad_wide: headblock


def fallback_reason(case, terms):
    """The first condition of launch_grad_wide's `headblock` that fails."""
    hs = case.hidden
    if terms != 3:
        return 'terms == 1'
    if len(hs) < 2:
        return 'one layer'
    if hs[-2] > 256:
        return 'width > 256'
    assert hs[-1] > WH_KMAX
    return 'K > 8'


def chunks_of(rows, R):
    return [min(R, rows - r0) for r0 in range(0, rows, R)]                                 # launch_grad_wide: the chunk walk


def launches(case, R=None):
    """Every launch of one gradient of `case` behind the weight preparation, in order.  R: the layout's chunk rows where it was
    made for another data set (set_data keeps it while E is unchanged), else what this case's own first call lays out."""
    hs, E, L = case.hidden, case.E, len(case.hidden)
    terms = 1 if case.kernel == X1 else 3
    assert case.kernel in (X3, X1)
    if R is None:
        R = layout_rows(hs, E, case.N, case.chunk_rows)
    rows = case.window[1] if case.window else case.N                                       # gp.N under a window (launch_grad_wide, launch_grad)
    wp = [up8(w) for w in hs]
    fin = [case.F] + list(hs[:-1])
    maxwp = max(wp)
    b_off, w_off, d, dp = offsets(case)
    H = [E * R * sum(wp[:l]) for l in range(L)]                                            # launch_grad_wide: H, tmp
    tmp = [E * R * sum(wp), E * R * sum(wp) + E * R * maxwp]
    hb = headblock_of(case, terms)
    act = case.act
    out = []
    for chunk, Rc in enumerate(chunks_of(rows, R)):
        for l in range(L - (1 if hb else 0)):                                              # layer_fwd
            last = l + 1 == L
            out.append(mm3('fwd-noact' if last else 'fwd', 'none' if last else act, Rc, hs[l], fin[l], wp[l], R * wp[l], H[l],
                           False, False, E, terms, chunk, l))
        if hb:                                                                             # MILE_HB, k_wide_headblock_reduce
            nblk = (Rc + HB_ROWS - 1) // HB_ROWS
            out.append(dict(kind='headblock', K=hs[-1], WFULL=hs[-2] == 256, nblk=nblk, last_rows=Rc - HB_ROWS * (nblk - 1),
                            grid=(nblk, E), accumulate=chunk != 0, chunk=chunk, rows=Rc))
            out.append(dict(kind='reduce', nblk=nblk, accumulate=chunk != 0, chunk=chunk))
            pp, ltop = 1, L - 2
        else:
            out.append(dict(kind='head', reason=fallback_reason(case, terms), task=case.task, first_chunk=chunk == 0, chunk=chunk,
                            rows=Rc))
            pp, ltop = 0, L - 1
        for l in range(ltop, -1, -1):                                                      # layer_dw, layer_dh
            out.append(mm3('dw', 'none', fin[l], hs[l], Rc, hs[l], dp, w_off[l], chunk != 0, True, E, terms, chunk, l))
            if l > 0:
                out.append(mm3('dh', act, Rc, fin[l], hs[l], wp[l - 1], R * wp[l - 1], tmp[pp], False, False, E, terms, chunk, l))
                pp ^= 1
    return out


def mixed(case):
    """The per-call memset of the two dZ buffers (launch_grad_wide: `mixed`)."""
    wp = [up8(w) for w in case.hidden]
    return any(wp[l] != wp[0] for l in range(1, len(wp) - 1))


def lds_bytes():
    """MMLayout<MM_A_MK, MM_B_T3_NK, TERMS, 32>::BYTES, what mile_grad_launch_info reports for the path (shape_wide): two
    row-major-K images of 128 rows x 256 bytes (mile_mm3.h:105-116)."""
    rowk = TILE * 256
    return max(2 * rowk, 4 * 32 * 68 * 4)


# ---- cells ---------------------------------------------------------------------------------------------------------------------------

ACTS = ('relu', 'tanh', 'sigmoid')
SHAPES = ('one ragged tile', 'whole tiles', 'several, ragged last')
NK = ('nk 1', 'nk 2', 'nk >= 3')
LASTK = ('last 32', 'last 17..31', 'last <= 16')
LAST_ROWS = ('< 4', '% 4 != 0', '% 4 == 0')


def shape(n):
    return SHAPES[1] if n % TILE == 0 else (SHAPES[0] if n < TILE else SHAPES[2])


def kshape(ln):
    return (NK[min(ln['nk'], 3) - 1], LASTK[0] if ln['last'] == KC else (LASTK[1] if ln['last'] > KSTEP else LASTK[2]))


def last_rows_class(n):
    return LAST_ROWS[0] if n < HB_WAVES else (LAST_ROWS[1] if n % HB_WAVES else LAST_ROWS[2])


def _enumerate_cells():
    cells = []
    # the epilogue: (form, activation, FULL) of the three-term form; the K-wide forward is never FULL at <= 16 outputs
    for f in ('fwd', 'dh'):
        cells += [('mm3', f, a, full, 3) for a in ACTS for full in (False, True)]
    cells += [('mm3', 'fwd-noact', 'none', False, 3)] + [('mm3', 'dw', 'none', full, 3) for full in (False, True)]
    # the one-term form: ReLU only (its oracle), one cell per (form, FULL)
    cells += [('mm3', f, 'relu', full, 1) for f in ('fwd', 'dh') for full in (False, True)]
    cells += [('mm3', 'fwd-noact', 'none', False, 1)] + [('mm3', 'dw', 'none', full, 1) for full in (False, True)]
    cells += [('dw-accum', acc, full, 3) for acc in (False, True) for full in (False, True)]
    cells += [('dw-accum', True, full, 1) for full in (False, True)]
    cells += [('dw-cvec', why, acc) for why in ('vec', 'ldc', 'base') for acc in (False, True)]
    # rows, columns, K: each against the form
    for f in ('fwd', 'dh', 'dw'):
        cells += [('m-shape', f, s) for s in SHAPES] + [('n-shape', f, s) for s in SHAPES]
    cells += [('m-shape', 'fwd-noact', s) for s in SHAPES] + [('n-shape', 'fwd-noact', SHAPES[0])]
    cells += [('n % 4 != 0', f) for f in ('fwd', 'fwd-noact', 'dh', 'dw')]
    cells += [('k-shape', f, nk, lk) for f in ('fwd', 'fwd-noact', 'dh', 'dw') for nk in NK for lk in LASTK]
    # XCD placement
    for f in ('fwd', 'dh'):
        cells += [('xcd', f, 0, full) for full in (False, True)]
        cells += [('xcd', f, 1, full, rem) for full in (False, True) for rem in ('whole groups of 8', 'M tiles beyond')]
    cells += [('xcd', 'fwd-noact', 0, False)]
    cells += [('xcd', 'dw', x, full) for x in (0, 2) for full in (False, True)]
    cells += [('colsum', mt, acc) for mt in ('M tiles == 1', 'M tiles >= 2') for acc in (False, True)]
    # the head
    cells += [('headblock', K, wfull) for K in range(1, WH_KMAX + 1) for wfull in (False, True)]
    cells += [('headblock-rows', nb, lr) for nb in ('nblk 1', 'nblk >= 2') for lr in LAST_ROWS]
    cells += [('headblock-accum', acc, nb) for acc in (False, True) for nb in ('nblk 1', 'nblk >= 2')]
    cells += [('headblock-accum-rows', acc, lr) for acc in (False, True) for lr in LAST_ROWS]
    cells += [('fallback', r, t) for r in ('K > 8', 'width > 256', 'one layer', 'terms == 1') for t in ('classification', 'regr')]
    # the walk
    cells += [('walk', c) for c in ('one chunk', 'several, ragged last', 'last chunk < 128 rows')]
    cells += [('window', w) for w in ('none', 'unaligned interior', 'tail', 'longer than a chunk')]
    cells += [('mixed memset', m) for m in (False, True)]
    assert len(cells) == len(set(cells))
    return cells


CELLS = _enumerate_cells()

# What the layers above the library refuse: cell -> the refusing line.
UNREACHABLE = {
    ('fallback', 'K > 8', 'regr'): "mile_amd/spec.py:43-44: regression needs hidden_structure[-1] == 2 (mu, log sigma), and 2 <= WH_KMAX",
}


def cells_of(case, R=None):
    """The cells one gradient of `case` runs a launch in."""
    out = set()
    ls = launches(case, R)
    for ln in ls:
        if ln['kind'] == 'mm3':
            f = ln['form']
            out.add(('mm3', f, ln['act'], ln['FULL'], ln['terms']))
            if ln['terms'] == 3:
                out |= {('m-shape', f, shape(ln['M'])), ('n-shape', f, shape(ln['N'])), ('k-shape', f) + kshape(ln)}
                if ln['N'] % 4:
                    out.add(('n % 4 != 0', f))
                if ln['xcd'] == 1:
                    out.add(('xcd', f, 1, ln['FULL'], 'whole groups of 8'))                # ny >= 8: the first eight M tiles
                    if ln['ny'] % 8:
                        out.add(('xcd', f, 1, ln['FULL'], 'M tiles beyond'))
                else:
                    out.add(('xcd', f, ln['xcd'], ln['FULL']))
            if f == 'dw':
                if ln['terms'] == 3 or ln['accumulate']:
                    out.add(('dw-accum', ln['accumulate'], ln['FULL'], ln['terms']))
                if ln['terms'] == 3:
                    out.add(('dw-cvec', ln['why'], ln['accumulate']))
                    out.add(('colsum', 'M tiles == 1' if ln['ny'] == 1 else 'M tiles >= 2', ln['accumulate']))
        elif ln['kind'] == 'headblock':
            nb, lr = 'nblk 1' if ln['nblk'] == 1 else 'nblk >= 2', last_rows_class(ln['last_rows'])
            out |= {('headblock', ln['K'], ln['WFULL']), ('headblock-rows', nb, lr), ('headblock-accum', ln['accumulate'], nb),
                    ('headblock-accum-rows', ln['accumulate'], lr)}
        elif ln['kind'] == 'head':
            out.add(('fallback', ln['reason'], ln['task']))
    if case.kernel == X3:
        rows = case.window[1] if case.window else case.N
        ch = chunks_of(rows, R if R is not None else layout_rows(case.hidden, case.E, case.N, case.chunk_rows))
        if len(ch) == 1:
            out.add(('walk', 'one chunk'))
        else:
            if ch[-1] != ch[0]:
                out.add(('walk', 'several, ragged last'))
            if ch[-1] < TILE:
                out.add(('walk', 'last chunk < 128 rows'))
        if case.window is None:
            out.add(('window', 'none'))
        else:
            b, c = case.window
            if b + c == case.N:
                out.add(('window', 'tail'))
            elif b % 32 and (b + c) % 32:
                out.add(('window', 'unaligned interior'))
            if len(ch) > 1:
                out.add(('window', 'longer than a chunk'))
        out.add(('mixed memset', mixed(case)))
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------------

B4S = (256, 256, 7)
CASES = [
    # the 256-wide nets: FULL products, the WFULL head block
    _c('w256-n256', 54, B4S, 'relu', 'classification', 256),
    _c('w256-n300', 54, B4S, 'relu', 'classification', 300),
    _c('w256-n300-rows128', 54, B4S, 'relu', 'classification', 300, chunk_rows=128),        # 128, 128, 44: FULL + ACCUM
    _c('w256-n300-rows128-e8', 54, B4S, 'relu', 'classification', 300, E=8, chunk_rows=128),  # xcd_remap 2 on both
    _c('w256x4-n256', 54, (256,) * 4 + (7,), 'relu', 'classification', 256),
    _c('w256-n1152-tanh', 54, B4S, 'tanh', 'classification', 1152),                          # nine whole M tiles: FULL under placement 1
    # the issue's general shapes
    _c('w160-k12', 20, (160, 12), 'relu', 'classification', 200),
    _c('w96-k4', 7, (96, 4), 'relu', 'classification', 130),
    _c('w256-k8', 7, (256, 8), 'relu', 'classification', 130),
    _c('w129-127-regr', 5, (129, 127, 2), 'relu', 'regr', 300),
    _c('w264-regr', 9, (264, 264, 2), 'tanh', 'regr', 130),
    _c('f130-w128', 130, (128, 3), 'sigmoid', 'classification', 130),
    _c('w200-136-n1153', 13, (200, 136, 3), 'tanh', 'classification', 1153),
    _c('w200-136-n1153-rows1024', 13, (200, 136, 3), 'tanh', 'classification', 1153, chunk_rows=1024),
    _c('w200-136-n1153-rows576', 13, (200, 136, 3), 'tanh', 'classification', 1153, chunk_rows=576),   # 576, 576, 1
    _c('w96-k4-n513', 7, (96, 4), 'relu', 'classification', 513),                            # one row in the second head block
    _c('w129-128-k5-rows128', 5, (129, 128, 5), 'sigmoid', 'classification', 130, E=3, chunk_rows=128),   # dW base misaligned, ldc % 4 == 0; a last chunk of two rows
    _c('w256-96-k6', 40, (256, 96, 6), 'sigmoid', 'classification', 256),                    # dW: whole M tiles, one ragged N tile
    _c('mixed-pad', 13, (100, 50, 20, 3), 'tanh', 'classification', 300, E=3),
    # the remaining head blocks
    _c('w96-k1', 7, (96, 1), 'tanh', 'classification', 130),
    _c('w256-k1', 7, (256, 1), 'sigmoid', 'classification', 130),
    _c('w256-regr', 7, (256, 2), 'relu', 'regr', 130, prior='Laplace'),
    _c('w256-k3', 7, (256, 3), 'tanh', 'classification', 130),
    _c('w256-k4', 7, (256, 4), 'sigmoid', 'classification', 130),
    _c('w256-k5', 7, (256, 5), 'tanh', 'classification', 130),
    _c('w256-k6', 7, (256, 6), 'tanh', 'classification', 130),
    _c('w200-k7', 7, (200, 7), 'sigmoid', 'classification', 130),
    _c('w96-k8', 7, (96, 8), 'sigmoid', 'classification', 130),
    # the fallback head and every K walk: (F, (W1, Wlast, K > 8)) at N rows put F, W1 into the forward's K, Wlast into the K-wide
    # forward's and the dH's, K into the dH's and N into the dW's
    _c('kzoo-20', 20, (96, 20, 9), 'sigmoid', 'classification', 20),
    _c('kzoo-32', 32, (96, 32, 10), 'relu', 'classification', 32),
    _c('kzoo-40', 40, (100, 40, 11), 'tanh', 'classification', 44),
    _c('kzoo-50', 54, (127, 50, 13), 'sigmoid', 'classification', 50),
    _c('kzoo-64', 64, (96, 64, 16), 'relu', 'classification', 64),
    _c('kzoo-127', 13, (96, 127, 12), 'tanh', 'classification', 127),
    _c('w264-k3', 7, (264, 3), 'relu', 'classification', 128),                               # the K-wide forward on a whole M tile
    _c('one-layer-k5', 40, (5,), 'relu', 'classification', 130),
    _c('one-layer-regr', 9, (2,), 'relu', 'regr', 130),
    # row windows of w256-n300 (whole set in one chunk) and of its 128-row walk
    _c('w256-n300-win-interior', 54, B4S, 'relu', 'classification', 300, window=(13, 150)),
    _c('w256-n300-win-tail', 54, B4S, 'relu', 'classification', 300, window=(297, 3)),
    _c('w256-n300-rows128-win', 54, B4S, 'relu', 'classification', 300, chunk_rows=128, window=(13, 200)),
    # the one-term form (ReLU only)
    _c('bf16-w256-n256', 54, B4S, 'relu', 'classification', 256, kernel=X1),
    _c('bf16-w256-n300-rows128', 54, B4S, 'relu', 'classification', 300, chunk_rows=128, kernel=X1),
    _c('bf16-w129-127-regr', 5, (129, 127, 2), 'relu', 'regr', 300, kernel=X1),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
X3_CASES = [c for c in CASES if c.kernel == X3 and c.window is None]
WINDOW_CASES = [c for c in CASES if c.window is not None]
X1_CASES = [c for c in CASES if c.kernel == X1]


def base_of(case):
    """The case a window case is a window of."""
    return next(c for c in CASES if c.window is None and c[1:9] == case[1:9] and c.kernel == case.kernel)


# ---- problems --------------------------------------------------------------------------------------------------------------------

KINK = 3e-7                     # of the layer's largest |z|: tests/test_gpu_parity.py's figure for "within fp32 rounding of the kink"
SEED_TRIES = 10
# The first seed in 0..9 whose two-chain problem has no hidden pre-activation within KINK of zero, judged on the fp64 oracle, per
# ReLU net and N (first_clean_seed; tests/test_wide_schedule_host.py checks every entry).  Seed 0 wherever nothing is listed, and
# for every other activation.  No case masks a row.
SEEDS = {
    # (F, hidden, N): seed.  Near-kink counts of seeds 0..3: (54, (256, 256, 7)) at N = 256: 0 0 2 0, at N = 300: 0 0 0 1;
    # (54, (256,) * 4 + (7,), 256): 0 0 1 0; (5, (129, 127, 2), 300): 0 1 0 1; (7, (96, 4), 513): 0 1 0 0; (7, (264, 3), 128): 0 1 0 0
    (54, (256, 256, 7), 256): 0, (54, (256, 256, 7), 300): 0, (54, (256, 256, 256, 256, 7), 256): 0, (20, (160, 12), 200): 0,
    (7, (96, 4), 130): 0, (7, (256, 8), 130): 0, (5, (129, 127, 2), 300): 0, (7, (96, 4), 513): 0, (7, (256, 2), 130): 0,
    (32, (96, 32, 10), 32): 0, (64, (96, 64, 16), 64): 0, (7, (264, 3), 128): 0,
}


def net_of(case):
    return (case.F, case.hidden, case.act, case.task, case.prior)


def ospec_of(net):
    from oracle import mclmc_oracle as M
    F, hidden, act, task, prior = net
    return M.ModelSpec(F, tuple(hidden), activation=act, task=task, prior=prior, prior_scale=0.7 if prior == 'Laplace' else 1.0)


def seed_of(case):
    """The tabulated seed of a ReLU net with a hidden layer; 0 for everything else (no kink, or no hidden pre-activation)."""
    if case.act == 'relu' and len(case.hidden) > 1:
        return SEEDS[(case.F, case.hidden, case.N)]
    return 0


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


def problem(case):
    """(ospec, X, y, theta [E, d]): the two-chain problem of the case's seed, its two parameter rows tiled to E particles (particle
    e is chain e % 2), so the fp64 reference stays at two rows and the kink condition does not depend on E."""
    net = net_of(case)
    prob = draw(net, case.N, seed_of(case))
    theta = np.ascontiguousarray(np.tile(prob['theta0'], ((case.E + 1) // 2, 1))[:case.E])
    return ospec_of(net), prob['X'], prob['y'], theta


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


def reference_of(case):
    b, c = case.window if case.window else (0, 0)
    return reference(net_of(case), case.N, seed_of(case), b, c)


@lru_cache(maxsize=None)
def reference_bf16(net, N, seed):
    """(logp [2], g [2, d]) of oracle.logpost_and_grad_bf16 in fp64: the one-term form's recipe."""
    from oracle import mclmc_oracle as M
    ospec, prob = ospec_of(net), draw(net, N, seed)
    lp, g = M.logpost_and_grad_bf16(ospec, prob['theta0'].astype(np.float64), prob['X'], prob['y'])
    lp.setflags(write=False)
    g.setflags(write=False)
    return lp, g


def gradient_over(net, N, seed, rows):
    """The fp64 oracle's gradient over the rows `rows` (an index array), the prior counted once."""
    from oracle import mclmc_oracle as M
    ospec, prob = ospec_of(net), draw(net, N, seed)
    rows = np.asarray(rows, dtype=np.int64)
    return M.logpost_and_grad(ospec, prob['theta0'].astype(np.float64), prob['X'][rows], prob['y'][rows])[1]


def prior_gradient(net, N, seed):
    from oracle import mclmc_oracle as M
    return M.log_prior(ospec_of(net), draw(net, N, seed)['theta0'].astype(np.float64))[1]


# ---- mutants ---------------------------------------------------------------------------------------------------------------------

def schedule_mutants(case):
    """{name: (gradient [2, d], names of the leaves it touches)} of what a wrong schedule would return for `case`, from the fp64
    oracle: (a) the last K chunk of a dW dropped -- the last Rc % 32 rows of the last row chunk missing from the first layer's
    kernel; (b) the bias gradient of a layer whose dW has two or more M tiles counted once per tile; (c) the last chunk stored
    instead of accumulated; (d) the last `rows % 4` rows of the last head block dropped; (e) a window one row late.  Only what the
    case's schedule can get wrong is returned."""
    from oracle import mclmc_oracle as M
    net, N, seed = net_of(case), case.N, seed_of(case)
    ospec = ospec_of(net)
    ents = M.param_slices(ospec)
    begin, rows = case.window if case.window else (0, N)
    idx = np.arange(begin, begin + rows)
    g = gradient_over(net, N, seed, idx)
    every = [f'layer{l}.{p}' for l in range(len(case.hidden)) for p in ('bias', 'kernel')]
    ls = launches(case)
    ch = chunks_of(rows, layout_rows(case.hidden, case.E, N, case.chunk_rows))
    out = {}
    if ch[-1] % KC and ch[-1] > ch[-1] % KC:                                              # (a)
        k0, k1 = ents[0]['kernel']
        gm = g.copy()
        gm[:, k0:k1] = gradient_over(net, N, seed, idx[:len(idx) - ch[-1] % KC])[:, k0:k1]
        out['dw-last-k-chunk-dropped'] = (gm, ['layer0.kernel'])
    gp = prior_gradient(net, N, seed)
    for ln in ls:                                                                          # (b)
        if ln['kind'] == 'mm3' and ln['form'] == 'dw' and ln['ny'] >= 2 and ln['chunk'] == 0:
            b0, b1 = ents[ln['layer']]['bias']
            gm = g.copy()
            gm[:, b0:b1] = gp[:, b0:b1] + ln['ny'] * (g[:, b0:b1] - gp[:, b0:b1])
            out[f"bias-once-per-m-tile-layer{ln['layer']}"] = (gm, [f"layer{ln['layer']}.bias"])
    if len(ch) > 1:                                                                        # (c)
        out['last-chunk-stored'] = (gradient_over(net, N, seed, idx[len(idx) - ch[-1]:]), every)
    hbs = [ln for ln in ls if ln['kind'] == 'headblock']
    if hbs and hbs[-1]['last_rows'] % HB_WAVES and rows > hbs[-1]['last_rows'] % HB_WAVES:  # (d)
        out['head-block-tail-dropped'] = (gradient_over(net, N, seed, idx[:len(idx) - hbs[-1]['last_rows'] % HB_WAVES]), every)
    if case.window and begin + rows < N:                                                   # (e)
        out['window-one-row-late'] = (gradient_over(net, N, seed, idx + 1), every)
    return out

"""What run_lenet decides, restated, and the cases that put a launch into every cell of that schedule (no torch, no GPU;
tests/test_lenet_schedule_host.py proves the table on the CPU, tests/test_gpu_lenet_schedule.py runs it).

The path (mile_amd/csrc/mile_hip.hip: run_lenet; kernels in mile_lenet.h and mile_lenet_mfma.h): the images -- the data set's, or a
row window's: the window only moves run_lenet's X, y and N -- are walked in chunks of R.  Per chunk a grid of (nwg, E) workgroups,
nwg = ceil(Rc / ipw), ipw = 8 (lenet_f32) or 16 (lenet_bf16, lenet_bf16x3) images each, runs conv1, conv2, and for the gradient
conv2's dW, conv2's dX and conv1's dW; each dW leaves one partial per workgroup (part1 / part2) that k_conv_reduce adds into the
slab, storing in chunk 0 and accumulating afterwards (acc = chunk != 0).  lenet_f32 takes the direct kernels (k_conv5_fwd / _dx /
_dw, geometry 0 / 1 / 3 at compile time) unless MILE_LENET_GEMM is set, C > 16 or an LDS tile exceeds 150 KiB; then im2col +
SGEMM.  The MFMA forms (k_conv5m_fwd2x / _fwd / _dw / _dx2x / _dw2x, TERMS = 1 or 3) stage ni = lenet_ni_for(bytes per image) images
per barrier pair, refuse C > 4 and everything the direct form refuses, and run the Dense half on k_mm3 with the head padded to 8.

CELLS are projections of a launch, not the Cartesian product of its properties.  The pruning rule of tests/wide_schedule.py: a
property is crossed with another one only where one piece of code reads both.  The activation is read with the pooling crop in
every back end's tile loads and epilogues, so (back end, activation, which convolution crops) are cells; the chunk walk, nwg, the
short last workgroup and acc meet in the part / k_conv_reduce indexing, per back end; ni, the group's fill, the tile counts and the
odd sizes meet inside each MFMA kernel, so they are crossed with the launch kind and TERMS and not with each other; G, the idle
threads and the reduction rounds of k_conv5_dw follow from C alone, so each distinct G is one cell; the GEMM form is crossed with
why it was taken; the head with its padding (MFMA) or its exact width (f32); windows and E with the kernel.
"""
from __future__ import annotations

from collections import namedtuple
from functools import lru_cache

import numpy as np

# ---- constants of the code (tests/test_lenet_schedule_host.py parses them out of the sources) ------------------------------------
IPW_F32, IPW_MFMA = 8, 16       # run_lenet: ipw
NI_BYTES = 57344                # lenet_ni_for
NI_CAP = 4
LDS_LIMIT = 150 * 1024          # run_lenet: direct, the MFMA refusal
RG = 3                          # k_conv5_dw: groups reduced per round
NT = 256                        # threads of every convolution kernel
REDUCE_GRID = {1: 2, 2: 10}     # k_conv_reduce<<<dim3(2 | 10, E)>>> for conv1 | conv2
PAIR_ROUND = 8                  # cm_image_f: four waves take tile pairs (t, t + 4), t advancing by 8
WS_FLOATS = 1 << 30             # run_lenet: the workspace budget
EVAL_BLOCK = 256                # loglik_lenet: samples per run_lenet call
F32, BF16, X3 = 'lenet_f32', 'lenet_bf16', 'lenet_bf16x3'
WIDE_PRIOR = 1000.0             # tests/leaf_cases.py's figure: every leaf's gradient is the likelihood's

Case = namedtuple('Case', 'name C H W K act task prior N E chunk_rows window kernel gemm_env wide seed')


def _c(name, C, H, W, K=3, act='relu', task='classification', N=5, E=2, prior='Normal', chunk_rows=None, window=None, kernel=F32,
       gemm_env=False, wide=True, seed=0):
    return Case(name, C, H, W, K, act, task, prior, N, E, chunk_rows, window, kernel, gemm_env, wide, seed)


# ---- the schedule ------------------------------------------------------------------------------------------------------------------

def geometry(H, W):
    hp1, wp1 = H // 2, W // 2
    h2, w2 = hp1 - 4, wp1 - 4
    return dict(hp1=hp1, wp1=wp1, h2=h2, w2=w2, hp2=h2 // 2, wp2=w2 // 2, flat=(h2 // 2) * (w2 // 2) * 16)


def lds_direct(C, H, W):
    """The five LDS sizes of the direct kernels, in bytes (run_lenet: lds_f1 .. lds_w2)."""
    g = geometry(H, W)
    HW, P1, HW2, KT1 = H * W, g['hp1'] * g['wp1'], g['h2'] * g['w2'], 25 * C
    return dict(lds_f1=(25 * C * 8 + 8 + C * (H + 4) * (W + 4)) * 4,
                lds_w1=max(C * (H + 4) * (W + 4) + HW * 6, RG * (KT1 * 6 + 6)) * 4,
                lds_f2=(150 * 16 + 16 + 6 * P1) * 4,
                lds_x2=(2400 + (g['h2'] + 8) * (g['w2'] + 8) * 16) * 4,
                lds_w2=max(6 * P1 + HW2 * 16, RG * (2400 + 16)) * 4)


def backend(C, H, W, gemm_env=False):
    """(direct, reason, geo): the reason names the first condition of run_lenet's `direct` that fails."""
    lds = lds_direct(C, H, W)
    geo = 1 if (C, H, W) == (3, 32, 32) else (3 if (C, H, W) == (1, 28, 28) else 0)
    if gemm_env:
        return False, 'env', geo
    if C > 16:
        return False, 'C > 16', geo
    big = [k for k, v in lds.items() if v > LDS_LIMIT]
    if big:
        return False, max(big, key=lambda k: lds[k]), geo
    return True, 'direct', geo


def ni_for(per_img, terms):
    return max(1, min(NI_CAP, NI_BYTES // (terms * per_img)))                                # lenet_ni_for


def ni_of(H, W, terms):
    """(ni_f1, ni2, ni_x2) of run_lenet."""
    g = geometry(H, W)
    return (ni_for(((H + 4) * (W + 4) + 8) * 8, terms),
            ni_for((g['hp1'] * g['wp1'] + 8) * 16 + g['h2'] * g['w2'] * 32, terms),
            ni_for(((g['h2'] + 8) * (g['w2'] + 8) + 8) * 32, terms))


def up(v, m):
    return (v + m - 1) // m * m


def cm_lds_fwd(in4, H, W, pad, CIN, COUT, ni=1, terms=1):
    return max(terms * ni * ((H + 2 * pad) * (W + 2 * pad) + 8) * (8 if in4 else 16), 25 * CIN * COUT * 4)


def cm_lds_dx2x(Ho, Wo, CIN, COUT, ni=1, terms=1):
    return max(terms * ni * ((Ho + 8) * (Wo + 8) + 8) * 32, 25 * CIN * COUT * 4)


def cm_lds_dw2x(H, W, pad, terms=1):
    Ho, Wo = H + 2 * pad - 4, W + 2 * pad - 4
    npairs = Ho * ((Wo + 1) // 2)
    return max(terms * (up(((H + 2 * pad) * (W + 2 * pad) + 8) * 8, 16) + up(npairs, 32) * 32), 4 * (8 + 1) * 64 * 16)


def cm_lds_dw(in4, H, W, pad, ni=1, terms=1):
    pb, ns = (8, 30) if in4 else (16, 50)
    Ho, Wo = H + 2 * pad - 4, W + 2 * pad - 4
    tiles = terms * (ni * up(((H + 2 * pad) * (W + 2 * pad) + 8) * pb, 16) + up(ni * Ho * Wo, 32) * 32)
    return max(tiles, 4 * ((ns + 3) // 4 + 1) * 64 * 16)


def mfma_lds(C, H, W, terms):
    """The five cm_lds_* sizes the MFMA launches take, and ldm_w1, which only the refusal reads."""
    g = geometry(H, W)
    ni_f1, ni2, ni_x2 = ni_of(H, W, terms)
    return dict(ldm_f1p=cm_lds_fwd(True, H, W, 2, C, 6, ni_f1, terms), ldm_f2=cm_lds_fwd(False, g['hp1'], g['wp1'], 0, 6, 16, ni2, terms),
                ldm_x2p=cm_lds_dx2x(g['h2'], g['w2'], 6, 16, ni_x2, terms), ldm_w1p=cm_lds_dw2x(H, W, 2, terms),
                ldm_w2=cm_lds_dw(False, g['hp1'], g['wp1'], 0, ni2, terms), ldm_w1=cm_lds_dw(True, H, W, 2))


def mfma_refused(C, H, W, terms, gemm_env=False):
    return (not backend(C, H, W, gemm_env)[0]) or C > 4 or max(mfma_lds(C, H, W, terms).values()) > LDS_LIMIT


def conv_tiles(H, W):
    """Per MFMA launch kind: Ho, Wo of the product, TX and the 16-row tiles of one image.  f1: k_conv5m_fwd2x on the image (pixel
    pairs: 16 columns per tile), c2: k_conv5m_fwd on conv2's output, dx: k_conv5m_dx2x on conv2's input (pairs along the width)."""
    g = geometry(H, W)
    out = {'f1': dict(Ho=H, Wo=W, TX=(W + 15) // 16), 'c2': dict(Ho=g['h2'], Wo=g['w2'], TX=(g['w2'] + 7) // 8)}
    for k in out.values():
        k['ntiles'] = (k['Ho'] + 1) // 2 * k['TX']
    W2 = (g['wp1'] + 1) // 2
    out['dx'] = dict(Ho=g['hp1'], Wo=g['wp1'], TX=W2, ntiles=(g['hp1'] * W2 + 15) // 16)
    return out


def dw_threads(CIN):
    """k_conv5_dw's thread map: K5, G, idle threads, reduction rounds and ng of the last round."""
    K5 = 5 * CIN
    G = NT // K5
    rounds = (G - 1 + RG - 1) // RG
    return dict(K5=K5, G=G, idle=NT - K5 * G, rounds=rounds, last_ng=(G - 1) - RG * (rounds - 1) if rounds else 0)


def reduce_passes(conv, C):
    per = (25 * C * 6 + 6) if conv == 1 else 2400 + 16
    return (per + REDUCE_GRID[conv] * NT - 1) // (REDUCE_GRID[conv] * NT)


def chunk_rows_of(case, rows, grad=True):
    """R of run_lenet for `rows` images (the window's count under a window): what 2^30 floats hold, then MILE_GEMM_ROWS."""
    g = geometry(case.H, case.W)
    mfma = case.kernel != F32
    direct = backend(case.C, case.H, case.W, case.gemm_env)[0]
    HW, P1, HW2 = case.H * case.W, g['hp1'] * g['wp1'], g['h2'] * g['w2']
    n_a1, n_p1, n_col2, n_a2, n_p2 = 6 * HW, 6 * P1, 150 * HW2, 16 * HW2, g['flat']
    w_f2, w_out = (88, up(case.K, 8)) if mfma else (84, case.K)
    per = n_a1 + n_p1 + (0 if direct else n_col2) + n_a2 + n_p2 + 120 + w_f2 + w_out
    if grad:
        per += w_f2 + 120 + n_p2 + n_p1 + (0 if direct else n_a2 + n_a1)
    shared = 0 if direct else 25 * case.C * HW
    R = max(1, min(WS_FLOATS // (case.E * per + shared), rows))
    if case.chunk_rows is not None:
        R = max(1, min(int(case.chunk_rows), rows))                                          # gemm_rows_hook
    return R


def rows_of(case):
    return case.window[1] if case.window else case.N


def walk(case):
    """[(Rc, nwg, images in the last workgroup, acc)] per chunk."""
    rows, ipw = rows_of(case), IPW_F32 if case.kernel == F32 else IPW_MFMA
    R = chunk_rows_of(case, rows)
    out = []
    for chunk, r0 in enumerate(range(0, rows, R)):
        Rc = min(R, rows - r0)
        nwg = (Rc + ipw - 1) // ipw
        out.append((Rc, nwg, Rc - ipw * (nwg - 1), int(chunk != 0)))
    return out


def workgroup_sizes(case):
    """The image counts of all workgroups of all chunks."""
    ipw = IPW_F32 if case.kernel == F32 else IPW_MFMA
    return [n for _, nwg, last, _ in walk(case) for n in [ipw] * (nwg - 1) + [last]]


def groups(nimgs, ni):
    """The barrier pairs of one workgroup of nimgs images: their image counts."""
    return [min(ni, nimgs - b) for b in range(0, nimgs, ni)]


def plan(case):
    """Everything above for one case, for the tests' messages and the note."""
    terms = 3 if case.kernel == X3 else 1
    direct, reason, geo = backend(case.C, case.H, case.W, case.gemm_env)
    p = dict(geometry(case.H, case.W), direct=direct, reason=reason, geo=geo, lds=lds_direct(case.C, case.H, case.W), walk=walk(case),
             R=chunk_rows_of(case, rows_of(case)), w_out=up(case.K, 8) if case.kernel != F32 else case.K)
    if case.kernel == F32:
        if direct:
            p.update(dw1=dw_threads(case.C), dw2=dw_threads(6), reduce1=reduce_passes(1, case.C), reduce2=reduce_passes(2, case.C))
    else:
        ni = dict(zip(('f1', 'c2', 'dx'), ni_of(case.H, case.W, terms)))
        p.update(terms=terms, ni=ni, ldm=mfma_lds(case.C, case.H, case.W, terms), refused=mfma_refused(case.C, case.H, case.W, terms, case.gemm_env),
                 tiles=conv_tiles(case.H, case.W),
                 groups={k: sorted({(len(groups(n, v)), groups(n, v)[-1]) for n in workgroup_sizes(case)}) for k, v in ni.items()})
    return p


# ---- cells ---------------------------------------------------------------------------------------------------------------------------

ACTS = ('relu', 'tanh', 'sigmoid')
BACKENDS = ('f32-direct', 'f32-gemm', BF16, X3)
MFMA = (BF16, X3)
KINDS = ('f1', 'c2', 'dx')
CROPS = ('conv1 crops', 'conv2 crops')
HEADS = ('regr', 'K < 8', 'K = 8', '8 < K < 16', 'K = 16')
TILES = ('below a round', 'one round', 'above a round')
WINDOWS = ('begins off a multiple of ipw', 'longer than a chunk', 'fewer rows than ipw')
G_OF_C = {c: NT // (5 * c) for c in range(1, 17)}


def backend_of(case):
    if case.kernel != F32:
        return case.kernel
    return 'f32-direct' if backend(case.C, case.H, case.W, case.gemm_env)[0] else 'f32-gemm'


def head_class(case):
    if case.task == 'regr':
        return HEADS[0]
    return HEADS[1] if case.K < 8 else HEADS[2] if case.K == 8 else HEADS[3] if case.K < 16 else HEADS[4]


def _enumerate_cells():
    cells = []
    cells += [('act', b, a, crop) for b in BACKENDS for a in ACTS for crop in CROPS]
    for b in BACKENDS:
        cells += [('chunks', b, n) for n in ('1', '2', '>= 3')] + [('last chunk of one image', b)]
        if b != 'f32-gemm':                                                                  # the GEMM form has no workgroups
            cells += [('later chunk nwg', b, n) for n in ('1', '>= 2')] + [('last workgroup', b, f) for f in ('full', 'short')]
        cells += [('E', b, e) for e in ('1', '> 1')] + [('prior', b, p) for p in ('wide', 'Normal', 'Laplace')]
    for k in MFMA:
        for kind in KINDS:
            cells += [('ni', k, kind, ni, fill) for ni in (1, 2, 3, 4) for fill in ('full', 'short') if not (ni == 1 and fill == 'short')]
            cells += [('tiles per barrier pair', k, kind, t) for t in TILES]
            cells += [('Ho odd', k, kind)]
        cells += [('Wo % 8', k, r) for r in ('zero', 'ragged')]                              # k_conv5m_fwd on conv2's output
        cells += [('Wo % 16', k, r) for r in ('zero', 'ragged')]                             # k_conv5m_fwd2x on the image
        cells += [('Wo odd in a pair form', k, f) for f in ('fwd2x / dw2x', 'dx2x')]
        cells += [('channels', k, c) for c in (1, 2, 3, 4, 5)]
    cells += [('dw G', G) for G in sorted(set(G_OF_C.values()) | {NT // 30})]
    cells += [('dw idle threads', z) for z in ('zero', 'non-zero')]
    cells += [('dw last round ng', n) for n in (1, 2, 3)]
    cells += [('geo', g) for g in (0, 1, 3)]
    cells += [('conv1 reduce', p) for p in ('one pass', 'several')]
    cells += [('gemm form', r) for r in ('env', 'C > 16', 'lds_w1')]
    cells += [('lds bound', s) for s in ('1x73x73 direct', '1x74x74 gemm')]
    cells += [('head', f, h) for f in ('f32', 'mfma') for h in HEADS]
    cells += [('window', k, w) for k in (F32, BF16, X3) for w in WINDOWS]
    assert len(cells) == len(set(cells))
    return cells


CELLS = _enumerate_cells()

# What cannot be reached: cell -> who refuses it, and how.  Five channels are refused twice: by the kernel's row in kGrad when the
# kernel is chosen (lenet_bf16_supported, the message below), and by run_lenet itself (RUN_LENET_REFUSAL) should that row ever let them by.
MFMA_REFUSAL = {BF16: 'LENET_BF16 is a kernel of MILE_MODEL_LENET and needs <= 4 image channels',
                X3: 'LENET_BF16X3 is a kernel of MILE_MODEL_LENET and needs <= 4 image channels'}
RUN_LENET_REFUSAL = {BF16: 'LENET_BF16 needs <= 4 image channels', X3: 'LENET_BF16X3 needs <= 4 image channels'}
UNREACHABLE = {
    ('dw idle threads', 'zero'): 'arithmetic, no layer: idle = 256 - 5 C (256 // (5 C)) and 5 does not divide 256, so k_conv5_dw always has idle threads',
    ('channels', BF16, 5): 'mile_set_grad_kernel (mile_hip.hip, kGrad: lenet_bf16_supported), when the engine is made: ' + MFMA_REFUSAL[BF16],
    ('channels', X3, 5): 'mile_set_grad_kernel (mile_hip.hip, kGrad: lenet_bf16_supported), when the engine is made: ' + MFMA_REFUSAL[X3],
}


def cells_of(case):
    """The cells one gradient of `case` runs a launch in."""
    b = backend_of(case)
    g = geometry(case.H, case.W)
    out = set()
    if case.window is None:
        if case.H % 2 or case.W % 2:
            out.add(('act', b, case.act, CROPS[0]))
        if g['h2'] % 2 or g['w2'] % 2:
            out.add(('act', b, case.act, CROPS[1]))
        w = walk(case)
        out.add(('chunks', b, '1' if len(w) == 1 else '2' if len(w) == 2 else '>= 3'))
        if len(w) > 1 and w[-1][0] == 1:
            out.add(('last chunk of one image', b))
        if b != 'f32-gemm':
            ipw = IPW_F32 if case.kernel == F32 else IPW_MFMA
            out |= {('later chunk nwg', b, '1' if nwg == 1 else '>= 2') for _, nwg, _, acc in w if acc}
            out |= {('last workgroup', b, 'full' if last == ipw else 'short') for _, _, last, _ in w}
        out.add(('E', b, '1' if case.E == 1 else '> 1'))
        out.add(('prior', b, 'wide' if case.wide else case.prior))
        out.add(('head', 'f32' if case.kernel == F32 else 'mfma', head_class(case)))
    else:
        begin, count = case.window
        ipw = IPW_F32 if case.kernel == F32 else IPW_MFMA
        if begin % ipw:
            out.add(('window', case.kernel, WINDOWS[0]))
        if len(walk(case)) > 1:
            out.add(('window', case.kernel, WINDOWS[1]))
        if count < ipw:
            out.add(('window', case.kernel, WINDOWS[2]))
    if case.kernel in MFMA:
        k = case.kernel
        terms = 3 if k == X3 else 1
        tiles = conv_tiles(case.H, case.W)
        for kind, ni in zip(KINDS, ni_of(case.H, case.W, terms)):
            for n in workgroup_sizes(case):
                gs = groups(n, ni)
                out.add(('ni', k, kind, ni, 'full' if gs[-1] == ni else 'short'))
                for nimg in gs:
                    t = nimg * tiles[kind]['ntiles']
                    out.add(('tiles per barrier pair', k, kind, TILES[0] if t < PAIR_ROUND else TILES[1] if t == PAIR_ROUND else TILES[2]))
            if tiles[kind]['Ho'] % 2:
                out.add(('Ho odd', k, kind))
        out.add(('Wo % 8', k, 'ragged' if g['w2'] % 8 else 'zero'))
        out.add(('Wo % 16', k, 'ragged' if case.W % 16 else 'zero'))
        if case.W % 2:
            out.add(('Wo odd in a pair form', k, 'fwd2x / dw2x'))
        if g['wp1'] % 2:
            out.add(('Wo odd in a pair form', k, 'dx2x'))
        out.add(('channels', k, case.C))
    elif b == 'f32-direct':
        for t in (dw_threads(case.C), dw_threads(6)):
            out |= {('dw G', t['G']), ('dw idle threads', 'non-zero' if t['idle'] else 'zero'), ('dw last round ng', t['last_ng'])}
        out.add(('geo', backend(case.C, case.H, case.W)[2]))
        out.add(('conv1 reduce', 'one pass' if reduce_passes(1, case.C) == 1 else 'several'))
        if (case.C, case.H, case.W) == (1, 73, 73):
            out.add(('lds bound', '1x73x73 direct'))
    else:
        out.add(('gemm form', backend(case.C, case.H, case.W, case.gemm_env)[1]))
        if (case.C, case.H, case.W) == (1, 74, 74):
            out.add(('lds bound', '1x74x74 gemm'))
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------------

def _walks(kernel, tag, C=2):
    """The chunk walks of one back end on 16 x 20 images: the issue's 20 + 17, three chunks with a last one of one image, two chunks
    of one workgroup each; and the whole set in one chunk with a full last workgroup."""
    ipw = IPW_F32 if kernel == F32 else IPW_MFMA
    return [_c(f'{tag}-walk-20+17', C, 16, 20, N=37, chunk_rows=20, kernel=kernel),
            _c(f'{tag}-walk-18+18+1', C, 16, 20, N=37, chunk_rows=18, kernel=kernel),
            _c(f'{tag}-walk-4+4+3', C, 16, 20, N=11, chunk_rows=4, E=3, kernel=kernel),
            _c(f'{tag}-full-workgroups', C, 16, 20, N=2 * ipw, E=1, kernel=kernel, seed=1)]


def _acts(kernel, tag, **kw):
    """Activation x crop: 13 x 17 crops a row and a column after conv1 (and conv2 sees 6 x 8 -> 2 x 4: none), 18 x 22 crops none
    after conv1 and a row and a column after conv2 (9 x 11 -> 5 x 7)."""
    out = []
    for a in ACTS:
        out.append(_c(f'{tag}-{a}-13x17', 2, 13, 17, act=a, N=9, kernel=kernel, **kw))
        out.append(_c(f'{tag}-{a}-18x22', 3, 18, 22, K=5, act=a, N=7, kernel=kernel, **kw))
    return out


def _mfma(kernel, tag):
    big = kernel == BF16            # terms = 1: ni < 4 needs images beyond 37 pixels a side
    out = _acts(kernel, tag) + _walks(kernel, tag)
    out += [
        # ni (f1, c2, dx); N = 12: every last group full, N = 5: short wherever ni > 1
        _c(f'{tag}-12x12-n12', 1, 12, 12, N=12, kernel=kernel),                                 # 4 4 4
        _c(f'{tag}-12x12-n5', 1, 12, 12, N=5, kernel=kernel),
        _c(f'{tag}-4x20x24', 4, 20, 24, K=4, N=19, kernel=kernel),
        _c(f'{tag}-1x16x32', 1, 16, 32, N=5, kernel=kernel),                                    # Wo % 16 == 0; conv2 4 x 12
        _c(f'{tag}-1x24x24', 1, 24, 24, N=4, kernel=kernel),                                    # conv2 8 x 8: Wo % 8 == 0
        _c(f'{tag}-1x14x13', 1, 14, 13, N=5, kernel=kernel),                                    # conv2's input 7 x 6, its output 3 x 2
        _c(f'{tag}-1x12x20-n1', 1, 12, 20, N=1, E=1, kernel=kernel),                            # c2: one image of 1 x 1 tiles
        # the head
        _c(f'{tag}-regr', 2, 13, 17, K=2, act='tanh', task='regr', N=9, kernel=kernel),
        _c(f'{tag}-k8', 1, 12, 12, K=8, N=12, kernel=kernel),
        _c(f'{tag}-k10', 1, 12, 12, K=10, N=12, kernel=kernel),
        _c(f'{tag}-k16', 1, 12, 12, K=16, N=12, kernel=kernel),
        # the standard priors
        _c(f'{tag}-normal', 3, 16, 20, K=5, act='tanh', N=40, kernel=kernel, wide=False),
        _c(f'{tag}-laplace', 3, 16, 20, K=2, act='tanh', task='regr', prior='Laplace', N=40, kernel=kernel, wide=False, seed=3),
        # windows of 40 images
        _c(f'{tag}-windows', 3, 16, 16, K=4, N=40, kernel=kernel, seed=2),
        _c(f'{tag}-win-10+16', 3, 16, 16, K=4, N=40, window=(10, 16), kernel=kernel, seed=2),
        _c(f'{tag}-win-3+9', 3, 16, 16, K=4, N=40, window=(3, 9), kernel=kernel, seed=2),
        _c(f'{tag}-windows-rows20', 3, 16, 16, K=4, N=40, chunk_rows=20, kernel=kernel, seed=2),
        _c(f'{tag}-win-5+33-rows20', 3, 16, 16, K=4, N=40, chunk_rows=20, window=(5, 33), kernel=kernel, seed=2),
    ]
    if big:
        out += [_c(f'{tag}-1x37x41', 1, 37, 41, N=5, kernel=kernel), _c(f'{tag}-1x37x41-n12', 1, 37, 41, N=12, kernel=kernel),   # 3 4 3
                _c(f'{tag}-1x37x54', 1, 37, 54, N=5, kernel=kernel), _c(f'{tag}-1x37x54-n12', 1, 37, 54, N=12, kernel=kernel),   # 3 3 2
                _c(f'{tag}-1x37x60', 1, 37, 60, N=5, kernel=kernel), _c(f'{tag}-1x37x60-n12', 1, 37, 60, N=12, kernel=kernel, seed=1),   # 2 2 2
                _c(f'{tag}-1x37x84', 1, 37, 84, N=3, kernel=kernel)]                                                             # 1 1 1
    else:
        out += [_c(f'{tag}-1x36x36', 1, 36, 36, N=5, kernel=kernel),                                                             # 1 1 1
                _c(f'{tag}-2x22x22', 2, 22, 22, N=5, kernel=kernel), _c(f'{tag}-2x22x22-n12', 2, 22, 22, N=12, kernel=kernel),   # 3 4 2
                _c(f'{tag}-1x28x28', 1, 28, 28, K=10, N=5, kernel=kernel), _c(f'{tag}-1x28x28-n12', 1, 28, 28, K=10, N=12, kernel=kernel),   # 2 2 1
                _c(f'{tag}-1x26x26', 1, 26, 26, N=5, kernel=kernel), _c(f'{tag}-1x26x26-n12', 1, 26, 26, N=12, kernel=kernel),   # 2 3 2
                _c(f'{tag}-1x18x21', 1, 18, 21, N=5, kernel=kernel), _c(f'{tag}-1x18x21-n12', 1, 18, 21, N=12, kernel=kernel)]   # 4 4 3
    return out


CASES = (
    # lenet_f32, direct
    _acts(F32, 'f32') + _walks(F32, 'f32')
    # every distinct G of conv1's dW (C = 1 .. 16), on the smallest image and an odd one in turn
    + [_c(f'f32-c{C}', C, 12 if C % 2 else 13, 12 if C % 3 else 15, N=9, act=ACTS[C % 3]) for C in range(1, 17)]
    + [_c('f32-mnist', 1, 28, 28, K=10, N=9), _c('f32-cifar', 3, 32, 32, K=10, N=9, seed=1),
       _c('f32-regr', 2, 13, 17, K=2, act='tanh', task='regr', N=9),
       _c('f32-k8', 1, 12, 12, K=8, N=9), _c('f32-k10', 1, 12, 12, K=10, N=9), _c('f32-k16', 1, 12, 12, K=16, N=9),
       _c('f32-normal', 3, 16, 20, K=5, act='tanh', N=40, wide=False),
       _c('f32-laplace', 3, 16, 20, K=2, act='tanh', task='regr', prior='Laplace', N=40, wide=False, seed=3),
       _c('f32-windows', 3, 16, 16, K=4, N=40, seed=2), _c('f32-win-10+16', 3, 16, 16, K=4, N=40, window=(10, 16), seed=2),
       _c('f32-win-3+5', 3, 16, 16, K=4, N=40, window=(3, 5), seed=2),
       _c('f32-windows-rows20', 3, 16, 16, K=4, N=40, chunk_rows=20, seed=2), _c('f32-win-5+33-rows20', 3, 16, 16, K=4, N=40, chunk_rows=20, window=(5, 33), seed=2),
       _c('f32-1x73x73', 1, 73, 73, N=2, E=1, act='tanh')]
    # lenet_f32, im2col + SGEMM: by the environment, by C = 17, by the LDS bound
    + _acts(F32, 'gemm', gemm_env=True)
    + [_c('gemm-walk-20+17', 2, 16, 20, N=37, chunk_rows=20, gemm_env=True), _c('gemm-walk-4+4+3', 3, 16, 20, K=5, N=11, E=3, chunk_rows=4, gemm_env=True),
       _c('gemm-walk-18+18+1', 2, 16, 20, N=37, E=1, chunk_rows=18, gemm_env=True),
       _c('gemm-c17', 17, 12, 13, N=9, act='tanh'), _c('gemm-1x74x74', 1, 74, 74, N=2, E=1, act='tanh'),
       _c('gemm-normal', 3, 16, 20, K=5, act='tanh', N=40, wide=False, gemm_env=True),
       _c('gemm-laplace', 3, 16, 20, K=2, act='tanh', task='regr', prior='Laplace', N=40, wide=False, gemm_env=True, seed=3)]
    + _mfma(BF16, 'bf16') + _mfma(X3, 'x3')
)
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
FULL_CASES = [c for c in CASES if c.window is None]
WINDOW_CASES = [c for c in CASES if c.window is not None]


def base_of(case):
    """The case a window case is a window of."""
    return next(c for c in FULL_CASES if c[1:11] == case[1:11] and c[12:] == case[12:])


# ---- problems --------------------------------------------------------------------------------------------------------------------

KINK = 5e-6                     # tests/test_gpu_lenet_bf16x3.py::_assert_off_the_kink: of the Dense layer's largest |z|
SHARE = 0.5                     # every leaf's likelihood gradient is at least this share of the leaf's gradient


def ospec_of(case):
    from oracle import lenet_oracle as LN
    scale = WIDE_PRIOR if case.wide else (0.7 if case.prior == 'Laplace' else 1.0)
    return LN.LeNetSpec(case.C, case.H, case.W, case.K, activation=case.act, task=case.task, prior=case.prior, prior_scale=scale)


def _key(case):
    return (case.C, case.H, case.W, case.K, case.act, case.task, case.prior, case.wide, case.N, case.seed)


@lru_cache(maxsize=None)
def _draw(key):
    from oracle import lenet_oracle as LN
    C, H, W, K, act, task, prior, wide, N, seed = key
    scale = WIDE_PRIOR if wide else (0.7 if prior == 'Laplace' else 1.0)
    prob = LN.synthetic_problem(LN.LeNetSpec(C, H, W, K, activation=act, task=task, prior=prior, prior_scale=scale), N, 2, seed=seed)
    for k in ('X', 'y', 'theta0'):
        prob[k].setflags(write=False)
    return prob


def problem(case):
    """(ospec, X, y, theta [E, d]): oracle.lenet_oracle.synthetic_problem at two chains and the case's seed, the two parameter
    rows tiled to E particles (particle e is chain e % 2).  A window case has its base's data; no row is masked."""
    prob = _draw(_key(case))
    theta = np.ascontiguousarray(np.tile(prob['theta0'], ((case.E + 1) // 2, 1))[:case.E])
    return ospec_of(case), prob['X'], prob['y'], theta


def _rows(case):
    b, c = case.window if case.window else (0, case.N)
    return slice(b, b + c)


@lru_cache(maxsize=None)
def _reference(key, begin, count, recipe):
    from oracle import lenet_oracle as LN
    case = _c('ref', *key[:3], K=key[3], act=key[4], task=key[5], prior=key[6], wide=key[7], N=key[8], seed=key[9])
    ospec, prob = ospec_of(case), _draw(key)
    X, y = prob['X'][begin:begin + count], prob['y'][begin:begin + count]
    f = LN.logpost_and_grad_bf16 if recipe == 'bf16' else LN.logpost_and_grad
    lp, g = f(ospec, prob['theta0'].astype(np.float64), X, y)
    _, g32 = f(ospec, prob['theta0'], X, y)
    assert g.dtype == np.float64 and g32.dtype == np.float32
    for a in (lp, g, g32):
        a.setflags(write=False)
    return lp, g, g32


def reference_of(case, recipe=None):
    """(logp [2], g [2, d]) in fp64 and the gradient of the same restatement evaluated at float32, on the case's rows; the plain
    oracle, or logpost_and_grad_bf16 for lenet_bf16 (`recipe`: 'f64' / 'bf16' overrides).  Shared: read-only."""
    recipe = recipe or ('bf16' if case.kernel == BF16 else 'f64')
    sl = _rows(case)
    return _reference(_key(case), sl.start, sl.stop - sl.start, recipe)


def gradient_over(case, rows):
    """The fp64 oracle's gradient over the images `rows` (an index array) of the case's data, the prior counted once."""
    from oracle import lenet_oracle as LN
    prob = _draw(_key(case))
    rows = np.asarray(rows, dtype=np.int64)
    return LN.logpost_and_grad(ospec_of(case), prob['theta0'].astype(np.float64), prob['X'][rows], prob['y'][rows])[1]


def prior_gradient(case):
    from oracle import mclmc_oracle as M
    return M.log_prior(ospec_of(case), _draw(_key(case))['theta0'].astype(np.float64))[1]


def kink_margin(case):
    """The smallest Dense pre-activation of the case's rows as a share of its layer's largest (fp64); inf off ReLU."""
    if case.act != 'relu':
        return np.inf
    from oracle import lenet_oracle as LN
    prob = _draw(_key(case))
    _, c = LN.forward(ospec_of(case), prob['theta0'].astype(np.float64), prob['X'][_rows(case)], keep=True)
    return min(float(np.abs(c[k]).min() / np.abs(c[k]).max()) for k in ('zf1', 'zf2'))


def shares(case):
    """[2, leaves]: likelihood_share of every leaf on the case's rows."""
    from tests import leafcheck as L
    _, g, _ = reference_of(case, 'f64')
    return L.likelihood_share(g - prior_gradient(case), g, L.spec_leaves(ospec_of(case)))


# ---- mutants ---------------------------------------------------------------------------------------------------------------------

CONV_LEAVES = ['core.conv1.bias', 'core.conv1.kernel', 'core.conv2.bias', 'core.conv2.kernel']


def _crop_mutant(case, which):
    """The gradient with the pooling crop of conv `which` ignored in the backward pass: dz_from_pool without its
    `y < 2 Hq && x < 2 Wq` test reads dp[(y >> 1) * Wq + (x >> 1)] on the cropped row / column too -- the next pooled row's first
    entry for a cropped column, the row behind the image's last for a cropped row (taken from the image's first row here)."""
    from oracle import lenet_oracle as LN
    ospec, prob = ospec_of(case), _draw(_key(case))
    sl = _rows(case)
    real = LN._unpool
    Ht, Wt = (case.H, case.W) if which == 1 else (ospec.h2, ospec.w2)

    def leaky(g, H, W):
        out = real(g, H, W)
        if (H, W) == (Ht, Wt):
            Hq, Wq = H // 2, W // 2
            if W % 2:
                for y in range(2 * Hq):
                    out[..., y, W - 1, :] = 0.25 * g[..., (y // 2 + 1) % Hq, 0, :]
            if H % 2:
                for x in range(2 * Wq):
                    out[..., H - 1, x, :] = 0.25 * g[..., 0, x // 2, :]
        return out

    LN._unpool = leaky
    try:
        return LN.logpost_and_grad(ospec, prob['theta0'].astype(np.float64), prob['X'][sl], prob['y'][sl])[1]
    finally:
        LN._unpool = real


def schedule_mutants(case):
    """{name: (gradient [2, d], names of the leaves it touches)} of what a wrong schedule would return for `case`, on the fp64
    oracle: (a) the last chunk stored instead of accumulated (k_conv_reduce's `accumulate`; the conv leaves, and for all leaves the
    Dense half's); (b) the last image of a short ni group dropped (conv leaves); (c) the last, short workgroup dropped (conv
    leaves); (d) the bias gradients of the convolutions counted for one workgroup more than there are (the first workgroup's twice);
    (e) a cropped pooling row or column treated as present; (f) a window one image late.  Only what the case's schedule can get wrong."""
    ospec = ospec_of(case)
    leaves = {n: (o, o + int(np.prod(s))) for n, o, s in ospec.leaves()}
    every = list(leaves)
    sl = _rows(case)
    idx = np.arange(sl.start, sl.stop)
    g = gradient_over(case, idx)
    gp = prior_gradient(case)
    w = walk(case)
    ipw = IPW_F32 if case.kernel == F32 else IPW_MFMA
    has_wgs = backend_of(case) != 'f32-gemm'
    out = {}

    def only(leafnames, g_other):
        gm = g.copy()
        for n in leafnames:
            b, e = leaves[n]
            gm[:, b:e] = g_other[:, b:e]
        return gm

    if len(w) > 1:                                                                           # (a)
        out['last-chunk-stored'] = (gradient_over(case, idx[len(idx) - w[-1][0]:]), every)
    if case.kernel in MFMA:                                                                  # (b)
        terms = 3 if case.kernel == X3 else 1
        drop, r0 = [], 0
        ni = min(ni_of(case.H, case.W, terms)[1:])                                           # the backward launches: c2 (dW), dx
        for Rc, nwg, last, _ in w:
            for wg in range(nwg):
                n = ipw if wg + 1 < nwg else last
                if n % ni:
                    drop.append(r0 + wg * ipw + n - 1)
            r0 += Rc
        if drop and len(drop) < len(idx):
            out['short-group-last-image-dropped'] = (only(CONV_LEAVES, gradient_over(case, np.delete(idx, drop))), CONV_LEAVES)
    if has_wgs and w[-1][2] < ipw and len(idx) > w[-1][2]:                                   # (c)
        out['last-short-workgroup-dropped'] = (only(CONV_LEAVES, gradient_over(case, idx[:len(idx) - w[-1][2]])), CONV_LEAVES)
    if has_wgs:                                                                              # (d)
        first = gradient_over(case, idx[:min(ipw, w[0][0])]) - gp
        gm = g.copy()
        for n in ('core.conv1.bias', 'core.conv2.bias'):
            b, e = leaves[n]
            gm[:, b:e] += first[:, b:e]
        out['bias-one-workgroup-too-often'] = (gm, ['core.conv1.bias', 'core.conv2.bias'])
    if case.H % 2 or case.W % 2:                                                             # (e)
        out['crop-treated-as-present-conv1'] = (_crop_mutant(case, 1), ['core.conv1.bias', 'core.conv1.kernel'])
    if ospec.h2 % 2 or ospec.w2 % 2:
        out['crop-treated-as-present-conv2'] = (_crop_mutant(case, 2), CONV_LEAVES)
    if case.window and sl.stop < case.N:                                                     # (f)
        out['window-one-image-late'] = (gradient_over(case, idx + 1), every)
    return out

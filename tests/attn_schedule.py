"""What the launch of the three attention gradient kernels decides, restated, and the cases that put a launch into every cell of
that schedule (no torch, no GPU; tests/test_attn_schedule_host.py proves the table on the CPU, tests/test_gpu_attn_schedule.py
runs it).

The kernels (mile_amd/csrc/mile_attn.h: attn_body -> k_grad_attn<NHT, WL>; mile_attn_pre.h: attnp_body -> k_grad_attn_pre<NHT> and,
with WIDE, k_grad_attn_wide<NHT>): grid (S row ranges, E chains), 256 threads, one sequence at a time.  Per sequence: tokens and
e [Tp][C] staged, q | k | v = e W on 16 x 16 tiles (attn: nj 3 ND tiles round-robin over the four waves; streamed: 3 ND column blocks,
each over all nj row tiles), the attention forward and backward head by head with wave w owning heads w, w + 4, ..., the Dense tail
on vectors, dW_qkv on CT 3 ND tiles, and -- where the tables are parameters -- de on nj CT (attn) or CT (wide) tiles, scattered
into the slab row's token block by atomics after a zero-fill.  The streamed kernels keep every accumulator in the slab row: the
first sequence of a range stores, the later ones add, an empty range writes zeros.

CELLS are projections of a launch, not the Cartesian product of its properties.  The pruning rule of tests/wide_schedule.py: a
property is crossed with another one only where one piece of code reads both.  NHT, WL and the run kind pick the instantiation, so
they are crossed; the raggedness of hd is read with NHT in the dq / dKl tiles; the guards of attn_tile are read per product, so C, D
and hd each have their own cells per family and are not crossed with each other; head ownership meets dK's place (registers or the
wave's scratch) where a wave's second head must zero dKl again; the tile loops are crossed with the four-wave round only; the tail
with NP and the bias; rank1's walk with nb and na nb; the row ranges and the windows with the family, because attn and pre take S
from the whole data set and wide from the window.
"""
from __future__ import annotations

from collections import namedtuple
from functools import lru_cache

import numpy as np

# ---- constants of the code (tests/test_attn_schedule_host.py parses them out of the sources) --------------------------------------
NT = 256
MAX_T = 128                     # ATTN_MAX_T
MAX_K = 16                      # ATTN_MAX_K
MAX_NP = 2                      # ATTN_MAX_NP
LIMITS = {'attn': dict(C=64, D=64, P=64), 'pre': dict(C=192, D=128, P=128), 'wide': dict(C=192, D=128, P=128)}
LDS_MAX = 160 * 1024            # ATTN_LDS_MAX
RANGE_CAP, RANGE_MIN_ROWS = 64, 16          # attn_ranges
WIDE_MIN_ROWS = 8               # ATTN_WIDE_MIN_ROWS
N_CU = 256                      # an MI355X; the GPU test asserts the plan's S against grad_launch_info
NDW, NDP, NFW = 12, 8, 16       # attn_body: dW_qkv, de tiles and tail entries a thread keeps in registers
MAX_NHT = {'attn': 4, 'pre': 8, 'wide': 8}
FAMILIES = ('attn', 'pre', 'wide')
STREAMED = ('pre', 'wide')
KERNEL = {'attn': 'k_grad_attn', 'pre': 'k_grad_attn_pre', 'wide': 'k_grad_attn_wide'}
GRAD_KERNEL = {'attn': 'attn_f32', 'pre': 'attn_pre_f32', 'wide': 'attn_wide_f32'}
WIDE_PRIOR = 1000.0             # tests/leaf_cases.py ATTN_PRIOR_SCALE: every leaf's gradient is the likelihood's
NORMAL_PRIOR = 0.2

Case = namedtuple('Case', 'name family V T C H D K proj bias N E window prev seed prior_scale')


def _c(name, family, V, T, C, H, D, K=2, proj=(8,), bias=True, N=5, E=2, window=None, prev=None, seed=3, prior_scale=WIDE_PRIOR):
    return Case(name, family, V, T, C, H, D, K, tuple(proj), bool(bias), N, E, window, prev, seed, prior_scale)


def up(v, m):
    return (v + m - 1) // m * m


# ---- the schedule ------------------------------------------------------------------------------------------------------------------

def geometry(T, C, H, D):
    Tp, hd = up(T, 16), D // H
    return dict(Tp=Tp, nj=Tp // 16, hd=hd, NHT=(hd + 15) // 16, CT=(C + 15) // 16, ND=(D + 15) // 16)


def attn_vec_floats(Tp):
    return 5 * Tp + 10 * 64 + 16


def attn_scr_wave(Tp, hd):
    return 16 * Tp + (Tp * up(hd, 16) if hd > 16 else 0)


def attn_scr_floats(Tp, H, hd):
    return max(64 * Tp, min(H, 4) * attn_scr_wave(Tp, hd))


def attn_lds_bytes(T, C, H, D, wl):
    Tp, hd = up(T, 16), D // H
    return ((C * 3 * D if wl else 0) + Tp * 3 * D + attn_scr_floats(Tp, H, hd) + attn_vec_floats(Tp)) * 4


def attn_weights_in_lds(T, C, H, D):
    return attn_lds_bytes(T, C, H, D, True) <= LDS_MAX


def _in_limits(family, T, C, H, D, K, proj):
    lim = LIMITS[family]
    if not (1 <= T <= MAX_T and 1 <= C <= lim['C'] and 1 <= D <= lim['D'] and H >= 1 and D % H == 0 and 1 <= K <= MAX_K
            and len(proj) <= MAX_NP):
        return False
    return all(1 <= p <= lim['P'] for p in proj)


def attn_supported(T, C, H, D, K=2, proj=()):
    return _in_limits('attn', T, C, H, D, K, proj) and attn_lds_bytes(T, C, H, D, False) <= LDS_MAX


def attnp_vec(Tp, C, D, proj):
    """AttnPreVec.n: tok | obar | dobar | z0 z1 z2 | a0 a1 | zf | dv0 dv1 | lg."""
    p0, p1 = (proj[0] if len(proj) > 0 else 0), (proj[1] if len(proj) > 1 else 0)
    W = max(C, p0, p1)
    zf = p1 if len(proj) > 1 else (p0 if len(proj) > 0 else C)
    return Tp + 2 * D + C + p0 + p1 + p0 + p1 + zf + 2 * W + 16


def attnp_scr_wave(Tp, hd):
    return 17 * Tp + (Tp * up(hd, 16) if hd > 16 else 0)


def attnp_scr_floats(Tp, C, H, hd):
    return max(Tp * C, min(H, 4) * attnp_scr_wave(Tp, hd))


def attnp_lds_bytes(T, C, H, D, proj=()):
    Tp, hd = up(T, 16), D // H
    return (Tp * 3 * D + attnp_scr_floats(Tp, C, H, hd) + attnp_vec(Tp, C, D, proj)) * 4


def attnp_supported(T, C, H, D, K=2, proj=()):
    return _in_limits('pre', T, C, H, D, K, proj) and attnp_lds_bytes(T, C, H, D, proj) <= LDS_MAX


def supported(case):
    f = attn_supported if case.family == 'attn' else attnp_supported
    return f(case.T, case.C, case.H, case.D, case.K, case.proj)


def lds_bytes(case):
    if case.family == 'attn':
        return attn_lds_bytes(case.T, case.C, case.H, case.D, attn_weights_in_lds(case.T, case.C, case.H, case.D))
    return attnp_lds_bytes(case.T, case.C, case.H, case.D, case.proj)


def attn_ranges(n_cu, E, rows):
    want = (n_cu + max(E, 1) - 1) // max(E, 1)
    return max(1, min(RANGE_CAP, want, max(1, rows // RANGE_MIN_ROWS)))


def attn_wide_S_rows(n_cu, E, rows):
    want = (n_cu + max(E, 1) - 1) // max(E, 1)
    return max(1, min(want, max(1, rows // WIDE_MIN_ROWS)))


def rows_of(case):
    """(begin, count) of the rows one gradient of `case` reads."""
    return case.window if case.window else (0, case.N)


def launch(case, n_cu=N_CU):
    """S, the rows of the launch, rows_per and the row count of every range (launch_grad: attn and pre take S from the whole data
    set whatever the window, wide from the window's rows; the bodies: rows_per = ceil(N / S), range s = [s rows_per, ...) cut at N)."""
    rows = rows_of(case)[1]
    want = (n_cu + case.E - 1) // case.E
    if case.family == 'wide':
        S, floor_ = attn_wide_S_rows(n_cu, case.E, rows), max(1, rows // WIDE_MIN_ROWS)
        binds = want < floor_
    else:
        S, floor_ = attn_ranges(n_cu, case.E, case.N), max(1, case.N // RANGE_MIN_ROWS)
        binds = want < min(RANGE_CAP, floor_)
    rows_per = (rows + S - 1) // S
    spans = [(min(rows, s * rows_per), min(rows, min(rows, s * rows_per) + rows_per)) for s in range(S)]
    return dict(S=S, rows=rows, rows_per=rows_per, spans=spans, counts=[e - b for b, e in spans], want=want, want_binds=binds)


def head_owner(H):
    """{wave: the heads it runs, in order} (h = wave, wave + 4, ...)."""
    return {w: list(range(w, H, 4)) for w in range(4)}


def offsets(case):
    """The parameter offsets of layout_attn_model that the kernels' alignment depends on: g.emb (-1 for pre), and every leaf's."""
    C, D, K, b = case.C, case.D, case.K, int(case.bias)
    o, out = 0, {}

    def put(name, nb, nk):
        nonlocal o
        out['b_' + name] = o if (b and nb) else -1
        o += nb if b else 0
        out['k_' + name] = o
        o += nk

    put('k', D, C * D); put('o', C, D * C); put('q', D, C * D); put('v', D, C * D)
    if case.family != 'pre':
        put('emb', 0, case.V * C); put('pos', 0, case.T * C)
    put('c', K, (case.proj[-1] if case.proj else C) * K)
    for l, p in enumerate(case.proj):
        put(f'p{l}', p, (case.proj[l - 1] if l else C) * p)
    out['d'] = o
    out['emb'] = out.get('k_emb', -1)
    return out


def zero_fill(case):
    """k_grad_attn_wide's fill of the token block: (g.emb & 3, head floats, 16-byte stores, tail floats)."""
    n, emb = case.V * case.C, offsets(case)['emb']
    head = min(n, (4 - (emb & 3)) & 3)
    nq = (n - head) >> 2
    return emb & 3, head, nq, n - head - 4 * nq


def rank1_calls(case):
    """attnp_body's rank1 calls per sequence: (leaf, na, nb, dr, dc)."""
    PL = case.proj[-1] if case.proj else case.C
    calls = [('classifier.kernel', PL, case.K)]
    for l in reversed(range(len(case.proj))):
        calls.append((f'projection_{l}.kernel', case.proj[l - 1] if l else case.C, case.proj[l]))
    calls.append(('MDPA.out.kernel', case.D, case.C))
    return [(n, na, nb, NT // nb, NT % nb) for n, na, nb in calls]


def tile_loops(case):
    """{loop: tile count} of the loops that go round the four waves."""
    g = geometry(case.T, case.C, case.H, case.D)
    if case.family == 'attn':
        return {'qkv': g['nj'] * 3 * g['ND'], 'dW': g['CT'] * 3 * g['ND'], 'de': g['nj'] * g['CT']}
    out = {'qkv': 3 * g['ND'], 'dW': g['CT'] * 3 * g['ND']}
    if case.family == 'wide':
        out['de'] = g['CT']
    return out


LOOP_MOST = {'qkv': (MAX_T // 16) * 3 * 4, 'dW': 4 * NDW, 'de': 4 * NDP}       # attn: nj 8 x 3 x ND 4; the register arrays' capacity


def plan(case):
    g = geometry(case.T, case.C, case.H, case.D)
    p = dict(g, lds=lds_bytes(case), supported=supported(case), **launch(case), owner=head_owner(case.H), loops=tile_loops(case))
    if case.family == 'attn':
        p['WL'] = attn_weights_in_lds(case.T, case.C, case.H, case.D)
    else:
        p['rank1'] = rank1_calls(case)
    if case.family == 'wide':
        p['zero_fill'] = zero_fill(case)
    return p


# ---- cells ---------------------------------------------------------------------------------------------------------------------------

RUNS = ('grad', 'loglik', 'raw')
ZNZ = ('zero', 'non-zero')
HD_CLASSES = ('1', '2..3', '4..15', '16')
H_CLASSES = ('1', '2..3', '4', '5..7', '8', '> 8')
NJ_CLASSES = ('1', '2..7', '8')
K_CLASSES = ('1', '2..15', '16')
ROUNDS = ('below a round', 'one round', 'above a round')
MASKS = ('a fully padded row', 'a row with one real token', 'a pad id in mid-sequence', 'a full row', 'a repeated token', 'id V - 1')
RANGES = ('S = 1', 'a short last range', 'a range of one sequence', 'a range of two sequences', 'an empty last range without a window',
          'N < 16', 'E = 1', 'want binds')
WINDOWS = ('fewer rows than ranges', 'a window after a larger one', 'the full set after a window')
RANK1 = ('nb divides 256', 'nb does not divide 256', 'nb = 1', 'na nb < 256', 'na nb > 256')
DK = ('dK in registers', 'dK in scratch')


def _class(v, edges, names):
    for e, n in zip(edges, names):
        if v <= e:
            return n
    return names[-1]


def inst_cell(family, NHT, WL, run):
    return ('inst', family, NHT, WL, run) if family == 'attn' else ('inst', family, NHT, run)


def _enumerate_cells():
    cells = []
    for f in FAMILIES:
        for nht in range(1, MAX_NHT[f] + 1):
            for run in RUNS:
                cells += [inst_cell(f, nht, wl, run) for wl in ((True, False) if f == 'attn' else (None,))]
            if nht > 1:
                cells += [('hd % 16', f, nht, r) for r in ('zero', 'ragged')]
        cells += [('hd % 4', f, r) for r in ZNZ] + [('hd at NHT = 1', f, c) for c in HD_CLASSES]
        cells += [(p, f, r) for p in ('C % 4', 'C % 16', 'D % 16') for r in ZNZ]
        cells += [(p, f) for p in ('C < 4', 'D < 4', 'C < 16')]
        cells += [('T % 16', f, r) for r in ('zero', 'ragged')] + [('nj', f, c) for c in NJ_CLASSES] + [('T < 16', f), ('T = 1', f)]
        cells += [('H', f, c) for c in H_CLASSES] + [('two heads on one wave', f, w) for w in DK]
        cells += [('tiles', f, loop, r) for loop in (('qkv', 'dW', 'de') if f != 'pre' else ('qkv', 'dW')) for r in ROUNDS]
        cells += [('NP', f, n, 'bias' if b else 'no bias') for n in (0, 1, 2) for b in (True, False)]
        cells += [('K', f, c) for c in K_CLASSES] + [('widths at their maxima', f)]
        cells += [('mask', f, m) for m in MASKS] + [('ranges', f, r) for r in RANGES] + [('window', f, w) for w in WINDOWS]
        cells += [('prior', f, p) for p in ('wide', 'Normal 0.2')]
        if f in STREAMED:
            cells += [('rank1', f, r) for r in RANK1]
    cells += [('3 D % 4', 'attn', 'non-zero')]
    cells += [('tiles at their most', 'attn', loop) for loop in ('qkv', 'dW', 'de')]
    cells += [('zero-fill emb & 3', r) for r in range(4)] + [('zero-fill tail', r) for r in range(4)] + [('zero-fill', 'V C smaller than the head')]
    cells += [('bound', 'attn', b) for b in ('largest WL = true', 'WL = false one step of T on')]
    cells += [('bound', f, b) for f in FAMILIES for b in ('largest supported', 'refused one step of T on')]
    assert len(cells) == len(set(cells))
    return cells


CELLS = _enumerate_cells()

# What the two bounds of 160 KiB decide, by enumeration (tests/test_attn_schedule_host.py repeats the enumeration):
#   the on-chip geometry with the most LDS that still stages its weights, whose neighbour one 16-step of T on streams them;
#   per envelope, the geometry with the most LDS that is supported, and its neighbour one 16-step of T on, which is refused.
# (over T, C, H, D at no projection and two classes; ties in C, which the on-chip size without weights does not read, go to C = 9)
BOUND_WL = (112, 39, 2, 64)                 # T, C, H, D: 163 840 bytes with Wq | Wk | Wv, the bound itself; T = 128: 182 592 with, 152 640 without
BOUND_ATTN = (112, 9, 3, 63, (), 2)         # T, C, H, D, proj, K: 154 048 bytes without the weights; T = 128 needs 175 680
BOUND_STREAMED = (80, 4, 4, 104, (), 2)     # 163 840 bytes, the bound itself; T = 96 needs 196 416
REFUSAL = {'attn': 'AttentionClassifier: shape needs more than 160 KB of LDS',
           'pre': 'PretrainedAttentionClassifier: shape needs more than 160 KB of LDS',
           'wide': 'AttentionClassifier (wide): shape needs more than 160 KB of LDS'}
LIMIT_REFUSAL = {'attn': 'AttentionClassifier: qkv_dim <= 64 and n_heads dividing it'}

UNREACHABLE = {}
for _run in RUNS:
    UNREACHABLE[('inst', 'attn', 3, False, _run)] = (
        'arithmetic, nobody refuses: NHT = 3 is hd in 33..48; D = H hd <= 64 forces H = 1 and D <= 48, and at the corner T = 128, C = 64, '
        'D = 48 (attn_lds_bytes grows with each) the weights still fit: 4 (9216 + 18432 + 8192 + 1296) = 148 544 <= 163 840')
UNREACHABLE[('two heads on one wave', 'attn', DK[1])] = (
    'layout_attn_model (mile_hip.hip) when the engine is made: two heads on a wave is H >= 5, dK in scratch is hd >= 17, so D >= 85 > '
    'ATTN_MAX_D: ' + LIMIT_REFUSAL['attn'])
for _f in FAMILIES:
    for _loop in ('qkv', 'dW'):
        UNREACHABLE[('tiles', _f, _loop, ROUNDS[1])] = 'arithmetic, nobody refuses: the count is a multiple of 3 (q | k | v) and a round is 4 tiles'
    UNREACHABLE[('bound', _f, 'refused one step of T on')] = 'layout_attn_model (mile_hip.hip) when the engine is made: ' + REFUSAL[_f]


def mask_kinds(x, V):
    """The masking situations in the token rows x [n, T] (int)."""
    out = set()
    for r in np.asarray(x):
        real = r != 0
        if not real.any():
            out.add(MASKS[0])
        if real.sum() == 1:
            out.add(MASKS[1])
        nz = np.nonzero(real)[0]
        if len(nz) and (~real[:nz[-1]]).any():
            out.add(MASKS[2])
        if real.all():
            out.add(MASKS[3])
        ids = r[real]
        if len(np.unique(ids)) < len(ids):
            out.add(MASKS[4])
        if (r == V - 1).any() and V > 1:
            out.add(MASKS[5])
    return out


def eval_cells_of(case):
    """The two evaluation instantiations the case's geometry runs (pointwise_loglik and predict)."""
    g = geometry(case.T, case.C, case.H, case.D)
    wl = attn_weights_in_lds(case.T, case.C, case.H, case.D) if case.family == 'attn' else None
    return {inst_cell(case.family, g['NHT'], wl, r) for r in ('loglik', 'raw')}


def cells_of(case):
    """The cells one gradient of `case` runs a launch in."""
    f = case.family
    g, L = geometry(case.T, case.C, case.H, case.D), launch(case)
    T, C, H, D, K, hd, nht = case.T, case.C, case.H, case.D, case.K, g['hd'], g['NHT']
    wl = attn_weights_in_lds(T, C, H, D) if f == 'attn' else None
    out = {inst_cell(f, nht, wl, 'grad')}
    if nht > 1:
        out.add(('hd % 16', f, nht, 'ragged' if hd % 16 else 'zero'))
    else:
        out.add(('hd at NHT = 1', f, _class(hd, (1, 3, 15), HD_CLASSES)))
    out.add(('hd % 4', f, ZNZ[hd % 4 != 0]))
    out |= {('C % 4', f, ZNZ[C % 4 != 0]), ('C % 16', f, ZNZ[C % 16 != 0]), ('D % 16', f, ZNZ[D % 16 != 0])}
    out |= {c for c, on in ((('C < 4', f), C < 4), (('D < 4', f), D < 4), (('C < 16', f), C < 16), (('T < 16', f), T < 16), (('T = 1', f), T == 1)) if on}
    if f == 'attn' and (3 * D) % 4:
        out.add(('3 D % 4', 'attn', 'non-zero'))
    out |= {('T % 16', f, 'ragged' if T % 16 else 'zero'), ('nj', f, _class(g['nj'], (1, 7), NJ_CLASSES))}
    out.add(('H', f, _class(H, (1, 3, 4, 7, 8), H_CLASSES)))
    if H > 4:
        out.add(('two heads on one wave', f, DK[nht > 1]))
    for loop, n in tile_loops(case).items():
        out.add(('tiles', f, loop, ROUNDS[0] if n < 4 else ROUNDS[1] if n == 4 else ROUNDS[2]))
        if f == 'attn' and n == LOOP_MOST[loop]:
            out.add(('tiles at their most', 'attn', loop))
    out.add(('NP', f, len(case.proj), 'bias' if case.bias else 'no bias'))
    out.add(('K', f, _class(K, (1, 15), K_CLASSES)))
    lim = LIMITS[f]
    if C == lim['C'] and D == lim['D'] and len(case.proj) == MAX_NP and all(p == lim['P'] for p in case.proj):
        out.add(('widths at their maxima', f))
    if f in STREAMED:
        for _, na, nb, _, _ in rank1_calls(case):
            out.add(('rank1', f, RANK1[0] if NT % nb == 0 else RANK1[1]))
            if nb == 1:
                out.add(('rank1', f, RANK1[2]))
            if na * nb != NT:
                out.add(('rank1', f, RANK1[3] if na * nb < NT else RANK1[4]))
    b, n = rows_of(case)
    out |= {('mask', f, m) for m in mask_kinds(rows_x(case), case.V)}
    counts = L['counts']
    if L['S'] == 1:
        out.add(('ranges', f, RANGES[0]))
    if L['S'] > 1 and 0 < counts[-1] < L['rows_per']:
        out.add(('ranges', f, RANGES[1]))
    if 1 in counts:
        out.add(('ranges', f, RANGES[2]))
    if 2 in counts:
        out.add(('ranges', f, RANGES[3]))
    if case.window is None and counts[-1] == 0:
        out.add(('ranges', f, RANGES[4]))
    if case.window is None and case.N < 16:
        out.add(('ranges', f, RANGES[5]))
    if case.E == 1:
        out.add(('ranges', f, RANGES[6]))
    if L['want_binds']:
        out.add(('ranges', f, RANGES[7]))
    if case.window is not None:
        full = launch(case._replace(window=None))
        if n < full['S']:
            out.add(('window', f, WINDOWS[0]))
        if case.prev is not None and BY_NAME[case.prev].window is not None and BY_NAME[case.prev].window[1] > n:
            out.add(('window', f, WINDOWS[1]))
    elif case.prev is not None and BY_NAME[case.prev].window is not None:
        out.add(('window', f, WINDOWS[2]))
    out.add(('prior', f, 'wide' if case.prior_scale == WIDE_PRIOR else 'Normal 0.2'))
    if f == 'wide':
        a, _, _, tail = zero_fill(case)
        out |= {('zero-fill emb & 3', a), ('zero-fill tail', tail)}
        if case.V * C < (4 - a) & 3:
            out.add(('zero-fill', 'V C smaller than the head'))
    if f == 'attn' and (T, C, H, D) == BOUND_WL:
        out.add(('bound', 'attn', 'largest WL = true'))
    if f == 'attn' and (T - 16, C, H, D) == BOUND_WL:
        out.add(('bound', 'attn', 'WL = false one step of T on'))
    if (T, C, H, D, case.proj, K) == (BOUND_ATTN if f == 'attn' else BOUND_STREAMED):
        out.add(('bound', f, 'largest supported'))
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------------

def _family(f):
    """The cases of one family; V, T, C, H, D then keywords.  The shapes are the smallest that reach a cell."""
    big = f != 'attn'
    out = []

    def add(name, *a, **k):
        out.append(_c(f'{f}-{name}', f, *a, **k))

    # head widths at NHT = 1, the product guards below 4 and below 16, the head counts, the tails
    add('hd1-h4', 30, 9, 6, 4, 4, proj=(), bias=False)                   # C % 4 = 2, D % 16, T < 16
    add('hd3-h2', 30, 9, 7, 2, 6, proj=(5,), bias=False, N=12)           # 3 D % 4 = 2, C % 4 = 3
    add('hd5-h3', 31, 20, 10, 3, 15, K=3, proj=(6, 5), bias=False, E=3)  # hd % 4 = 1, H in 2..3; the third particle repeats chain 0
    add('hd16-h1', 30, 16, 16, 1, 16, proj=(), bias=True)                # every product on whole tiles
    add('hd2-h5', 20, 13, 8, 5, 10, proj=(9, 7), bias=True)              # waves 0 owns heads 0 and 4
    add('hd2-h8', 20, 17, 12, 8, 16, K=16, proj=(4,))                    # every wave owns two heads
    add('hd1-h12', 20, 24, 5, 12, 12, K=5, proj=(3,))                    # three heads a wave
    add('c1-d1', 2, 3, 1, 1, 1, K=2, proj=(1,), N=7)                     # C = D = P = 1: V C = 2
    if f == 'wide':                                                      # the alignments of the token block's zero-fill
        add('c3-d3', 9, 5, 3, 3, 3, K=4, proj=(), N=6)                   # emb & 3 = 0 with a bias
        add('c2-d4-bias', 2, 4, 1, 1, 4, K=3, proj=(2,), N=7)            # emb & 3 = 1, a head of 3 floats and V C = 2
        add('c3-d4', 9, 5, 3, 2, 4, K=3, proj=(2,), N=7)                 # emb & 3 = 3
    add('t1', 12, 1, 8, 2, 8, proj=(4,), N=6)                            # T = 1: one key, the softmax is constant
    add('k1', 12, 6, 8, 2, 8, K=1, proj=(4,))                            # one class: the likelihood is constant
    add('n1-e1', 17, 11, 8, 2, 8, proj=(), N=1, E=1)                     # one sequence, one chain
    add('t37', 50, 37, 24, 4, 32, K=3, proj=(20, 12), N=9)               # nj = 3, T ragged, hd = 8
    add('t128', 60, 128, 20, 4, 16, proj=(8,), N=4)                      # nj = 8
    if f != 'pre':
        add('c64-d64', 40, 16, 64, 4, 64, K=16, proj=(64, 64), N=6)      # on chip: every width at its most; CT = ND = 4: wide's de loop is one round
    add('normal', 40, 12, 16, 4, 16, proj=(8,), N=24, prior_scale=NORMAL_PRIOR)
    # NHT > 1: hd a multiple of 16 and ragged, one head (two where the widths allow it)
    for nht in range(2, MAX_NHT[f] + 1):
        add(f'hd{16 * nht}', 25, 18, 12, 1, 16 * nht, proj=(8,), N=4)
        add(f'hd{16 * nht - 5}', 25, 19, 13, 1, 16 * nht - 5, K=3, proj=(), bias=nht % 2 == 0, N=4)
    if big:
        add('hd20-h5', 25, 21, 9, 5, 100, proj=(8,), N=4)                # a wave's second head zeroes dKl again
        add('widest', 40, 16, 192, 8, 128, K=16, proj=(128, 128), N=4)
    # the bounds of 160 KiB
    if f == 'attn':
        add('wl-last', 60, *BOUND_WL, proj=(16,), N=3)
        add('wl-first-off', 60, BOUND_WL[0] + 16, *BOUND_WL[1:], proj=(16,), N=3)
        add('most-tiles', 200, 128, 64, 8, 64, K=16, proj=(64, 64), N=3)
        add('hd64-t128', 60, 128, 64, 1, 64, proj=(16,), N=3)                    # <4, false>
        add('largest', 60, *BOUND_ATTN[:4], K=BOUND_ATTN[5], proj=BOUND_ATTN[4], N=3)
    else:
        add('largest', 60, *BOUND_STREAMED[:4], K=BOUND_STREAMED[5], proj=BOUND_STREAMED[4], N=3)
    # row ranges (T = 8: the restatement of 289 rows is a moment)
    r = dict(proj=(4,), seed=5)
    if f == 'wide':
        add('rows81', 40, 8, 9, 2, 8, N=81, **r)                         # S = 10, rows_per = 9: the tenth range is empty
        add('rows73', 40, 8, 9, 2, 8, N=73, **r)                         # 8 ranges of 9 and one of 1
        add('rows74-e1', 40, 8, 9, 2, 8, N=74, E=1, **r)                 # ... of 2
        add('rows40-e128', 40, 8, 9, 2, 8, N=40, E=128, **r)             # want = 2 < 40 / 8
    else:
        add('rows289', 40, 8, 9, 2, 8, N=289, **r)                       # S = 18, rows_per = 17: the eighteenth range is empty
        add('rows273', 40, 8, 9, 2, 8, N=273, **r)                       # 16 ranges of 17 and one of 1
        add('rows274-e1', 40, 8, 9, 2, 8, N=274, E=1, **r)               # ... of 2
        add('rows48-e128', 40, 8, 9, 2, 8, N=48, E=128, **r)             # want = 2 < 48 / 16
    # the stale-state sequence on one engine: the full set, a window, a smaller window with fewer distinct tokens, the full set
    s = dict(proj=(6,), N=160, seed=4)
    add('seq-full', 300, 12, 21, 4, 16, **s)                          # wide: a head of 3 floats and a tail of 1
    add('seq-win37', 300, 12, 21, 4, 16, window=(20, 37), prev=f'{f}-seq-full', **s)
    add('seq-win3', 300, 12, 21, 4, 16, window=(100, 3), prev=f'{f}-seq-win37', **s)
    add('seq-again', 300, 12, 21, 4, 16, prev=f'{f}-seq-win3', **s)
    return out


CASES = [c for f in FAMILIES for c in _family(f)]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
SEQUENCES = {f: [f'{f}-seq-full', f'{f}-seq-win37', f'{f}-seq-win3', f'{f}-seq-again'] for f in FAMILIES}
SINGLE_CASES = [c for c in CASES if c.prev is None and not c.name.endswith('seq-full')]
# the geometries whose evaluation kernels run: the first case of every reachable (family, NHT, WL)
EVAL_CASES = []
for _case in CASES:
    if not eval_cells_of(_case) <= {c for e in EVAL_CASES for c in eval_cells_of(e)}:
        EVAL_CASES.append(_case)
# an on-chip case also runs on k_grad_attn_wide
ALSO_WIDE = [c.name for c in CASES if c.family == 'attn' and c.prev is None and c.window is None and c.N <= 40 and c.E <= 3]

# What is zero analytically and so has no likelihood share: the key bias always (the softmax is shift-invariant per query row); every
# query and key leaf where a row has one key (T = 1); every leaf where there is one class (the log-softmax of one logit is 0).
KEY_BIAS = 'MDPA.key.bias'
QK_LEAVES = ('MDPA.query.bias', 'MDPA.query.kernel', 'MDPA.key.bias', 'MDPA.key.kernel')


def zero_leaves(case, names):
    if case.K == 1:
        return set(names)
    if case.T == 1:
        return set(QK_LEAVES) & set(names)
    return {KEY_BIAS} & set(names)


def library_refuses(family, V, T, C, H, D, K=2, proj=(), bias=True):
    """mile_create on the geometry (no GPU needed): (return code, the library's message)."""
    import ctypes
    from mile_amd import _lib
    cs = _lib.ModelSpecC()
    cs.in_features = T
    widths = list(proj) + [K]
    cs.n_layers = len(widths)
    for i, w in enumerate(widths):
        cs.widths[i] = w
    cs.task, cs.prior, cs.prior_scale, cs.use_bias = 1, 0, 1.0, int(bias)
    cs.model = _lib.MODEL_IDS[{'attn': 'attn', 'pre': 'attn_pretrained', 'wide': 'attn_wide'}[family]]
    cs.vocab_size, cs.ctx_len, cs.emb_size, cs.n_heads, cs.qkv_dim = V, T, C, H, D
    lib = _lib.load_library()
    h = ctypes.c_void_p()
    rc = lib.mile_create(ctypes.byref(cs), 0, ctypes.byref(h))
    msg = (lib.mile_last_error() or b'').decode() if rc != 0 else ''
    if rc == 0:
        lib.mile_destroy(h)
    return rc, msg, h.value


# the first geometry past each bound: (family, T, C, H, D, proj, K) -> refused with REFUSAL[family]; and what the limits refuse
REFUSED = [('attn', BOUND_ATTN[0] + 16) + BOUND_ATTN[1:]] + [(f, BOUND_STREAMED[0] + 16) + BOUND_STREAMED[1:] for f in STREAMED]
REFUSED_BY_LIMIT = [('attn', 21, 9, 5, 100, (8,), 2)]       # two heads on a wave with dK in scratch: pre-hd20-h5's geometry on chip


# ---- problems --------------------------------------------------------------------------------------------------------------------

# sharp_problem's scale on the query and key kernels where its default sqrt(2 C) leaves attention flat, searched in the order
# QK_LADDER on the fp64 restatement alone (tests/test_attn_schedule_host.py repeats the search): the first scale at which the
# thresholds of tests/test_leafcheck_host.py hold.  None: the default.
QK_LADDER = (None, 4.0, 6.0, 8.0, 12.0, 16.0, 24.0, 32.0)
QK_SCALE = {'wide-c3-d4': 4.0, 'attn-n1-e1': 6.0, 'pre-n1-e1': 6.0, 'wide-n1-e1': 6.0}


def flat_by_construction(case):
    """Cases no scale makes sharp: one key (T = 1), or an embedding of one number per position (C = 1: every score of a head is
    the product of two scalars, and a scale that spreads them past 1e-6 takes the largest logit past 80 or the share below 0.5)."""
    return case.T == 1 or case.C == 1


def prior_dominated(case):
    """The Normal(0.2) case of each family is there for the prior's path; at that scale the prior's gradient exceeds the likelihood's
    in most leaves (tests/test_leafcheck_host.py::test_old_attention_problems_are_prior_dominated), so the share condition is not its."""
    return case.prior_scale != WIDE_PRIOR


def qk_of(case):
    """The recorded scale of the case: a window case has its sequence's, an on-chip case run on the wide kernel its own."""
    return QK_SCALE.get((case.name if case.prev is None else SEQUENCES[case.family][0]).removesuffix('-on-wide'))


def spec_of(case):
    from mile_amd.spec import AttentionSpec, PretrainedAttentionSpec, WideAttentionSpec
    cls = {'attn': AttentionSpec, 'pre': PretrainedAttentionSpec, 'wide': WideAttentionSpec}[case.family]
    return cls(case.V, case.T, case.C, case.H, case.D, n_classes=case.K, projection_dim=case.proj, use_bias=case.bias, prior='Normal',
               prior_scale=case.prior_scale)


def _key(case):
    return (case.family, case.V, case.T, case.C, case.H, case.D, case.K, case.proj, case.bias, case.N, case.seed, case.prior_scale)


@lru_cache(maxsize=None)
def _draw(key, qk_scale):
    from tests import attn_pre_ref as RP
    from tests import attn_ref as RA
    case = _c('draw', *key[:7], proj=key[7], bias=key[8], N=key[9], seed=key[10], prior_scale=key[11])
    spec = spec_of(case)
    prob = (RP if case.family == 'pre' else RA).sharp_problem(spec, case.N, 2, case.seed, qk_scale)
    for k in ('X', 'x', 'y', 'theta0'):
        prob[k].setflags(write=False)
    return spec, prob


def rows_x(case):
    """The token rows [count, T] (int) one gradient of `case` reads: drawn without the parameters' spec (no import of mile_amd)."""
    b, n = rows_of(case)
    return _rows(case.T, case.V, case.K, case.N, case.seed)[b:b + n]


@lru_cache(maxsize=None)
def _rows(T, V, K, N, seed):
    from tests import attn_ref as RA

    class _S:                                           # what synthetic_problem's row draw reads
        context_len, vocab_size, n_classes, n_params = T, V, K, 0

        @staticmethod
        def leaves():
            return []

    x = RA.synthetic_problem(_S, N, 2, seed)['x']
    x.setflags(write=False)
    return x


def problem(case, qk_scale='recorded'):
    """tests/leaf_cases.AttnProblem of the case: sharp_problem at two chains under the case's prior, a window case on its base's
    data.  `P.rows` is the slice of the case's rows, `P.theta(E)` the two chains tiled to E particles (particle e is chain e % 2)."""
    from tests import leaf_cases as LC
    if qk_scale == 'recorded':
        qk_scale = qk_of(case)
    spec, prob = _draw(_key(case), qk_scale)
    P = LC.AttnProblem('pre' if case.family == 'pre' else 'attn', spec, prob)
    b, n = rows_of(case)
    P.rows = slice(b, b + n)
    P.theta = lambda E=case.E: np.ascontiguousarray(np.tile(prob['theta0'], ((E + 1) // 2, 1))[:E])
    return P


@lru_cache(maxsize=None)
def _reference(key, qk_scale, b, n):
    case = _c('ref', *key[:7], proj=key[7], bias=key[8], N=key[9], seed=key[10], prior_scale=key[11])
    P = problem(case, qk_scale)
    rows = slice(b, b + n)
    lp, g = P.ref(rows=rows)
    _, g32 = P.ref(np.float32, rows)
    for a in (lp, g, g32):
        a.setflags(write=False)
    return lp, g, g32


def reference_of(case):
    """(logp [2], g [2, d]) in fp64 and the gradient of the same restatement evaluated in float32, on the case's rows.  Shared:
    read-only."""
    return _reference(_key(case), qk_of(case), *rows_of(case))

"""What one launch of k_grad_narrow does, restated, one net per template instantiation, and the cases that put a workgroup into
every cell of its row walk (no torch, no GPU; tests/test_narrow_schedule_host.py proves the table on the CPU,
tests/test_gpu_narrow_schedule.py runs it).

The kernel (mile_amd/csrc/mile_grad_narrow.h, launched from mile_hip.hip and mile_narrow_part.hip): <NH, TH, TF> are the hidden
layers, the 16-wide tiles of the widest hidden layer and 1 (F <= 16) or 4 tiles of inputs; TH >= 3 keeps the weights in LDS (WL),
where the cross-wave reduction image of 64 NACC floats aliases them.  Grid (S, E): workgroup s walks the rows
[s rows_per, min(N, (s + 1) rows_per)) in 16-row tiles, wave w taking tiles w, w + nw, ...; a wave without a tile still joins the
reduction, a workgroup without one writes an all-zero slab.  Under a row window S is the full set's, nw and rows_per the window's.

A cell is a projection (as in tests/update_schedule.py): ('waves', 1..4), ('tiles', 0 / 1 / 2) of one wave of a workgroup that has
a tile (2 stands for two or more), ('last', 'full' / 'r1' / 'r15') for the launch's last tile, and ('empty',) for a workgroup without
any tile, which only a window produces.  A register form never has an idle wave in a one-workgroup launch (nw = min(4, tiles) there).

Problems come from oracle/mclmc_oracle.py alone (a ReLU net's hidden biases are made positive, so that no hidden unit is off on
every row: the gradient of such a unit is zero whatever the kernel masks).  The prior is Normal(0, 1000), so every leaf's gradient
is the likelihood's; the size of the parameters is the first of leaf_cases.THETA_LADDER, and the seed the first of
0 .. SEED_TRIES - 1, for which no hidden pre-activation of a ReLU net is within 3e-7 of its layer's largest, every leaf of both
chains has a likelihood share of at least leaf_cases.MIN_SHARE on every row set the case evaluates, the oracle evaluated at float32
is within 5e-6 of the whole gradient's largest entry (WHOLE_F32), no leaf's row sum cancels by more than 209x (CANCEL_MAX), and
every mutant of `mutant_misses` misses the per-leaf bound tenfold (`search`, which prints SCALES and SEEDS; the activation and the
rows stay as they are, unlike leaf_cases.deep_fcn_problem, because either
would move the case into another form or cell).
"""
from __future__ import annotations

from collections import namedtuple
from functools import lru_cache

import numpy as np

N_CU = 256                      # an MI355X
NRW_MAXW = 4                    # mile_grad_narrow.h (the host test reads both from the source)
NRW_TS = 20


# ---- the dispatch -------------------------------------------------------------------------------------------------------------

def supported(F, hs, task):
    """narrow_supported for an FCN with biases: hs as hidden_structure (the last entry is the output layer)."""
    nh = len(hs) - 1
    if nh < 1 or nh > 10 or F > 64:
        return False
    if any(w < 1 or w > (16 if nh > 3 else 64) for w in hs[:-1]):
        return False
    if nh > 3 and F > 16:
        return False
    K = hs[-1]
    if K < 1 or K > 16:
        return False
    return not (task == 'regr' and K != 2)


def tiles_hidden(hs):
    return (max(hs[:-1]) + 15) // 16


def instantiation(F, hs):
    """<NH, TH, TF> of launch_narrow."""
    return (len(hs) - 1, tiles_hidden(hs), 1 if F <= 16 else 4)


def weights_in_lds(inst):
    return inst[1] >= 3


FULL_INSTANTIATIONS = ([(nh, th, tf) for nh in (1, 2, 3) for tf in (1, 4) for th in (1, 2)] + [(nh, 1, 1) for nh in range(4, 11)]
                       + [(nh, th, tf) for nh in (1, 2, 3) for tf in (1, 4) for th in (3, 4)])
PART_INSTANTIATIONS = [i for i in FULL_INSTANTIATIONS if i[0] >= 2]         # a net with one hidden layer has no frozen layer


def nacc(nh, th, tf):
    """NarrowLayout::NACC: the floats per lane that a wave parks for the reduction."""
    return 4 * (tf * th + (nh - 1) * th * th + th) + (nh * th + 1) + 1


def layout_bytes(nh, th, tf):
    """NarrowLayout<NH, TH, TF, TH >= 3>::BYTES."""
    trans, red = NRW_MAXW * 16 * NRW_TS, 64 * nacc(nh, th, tf)
    hp = 16 * th
    sh, sl = hp + 4, 20
    wtot = 16 * tf * sh + 2 * (nh - 1) * hp * sh + hp * sl + 16 * sh
    return 4 * (trans + (max(wtot, red) if th >= 3 else red))


# ---- the schedule -------------------------------------------------------------------------------------------------------------

def splits(N_full, E, th, n_cu=N_CU):
    """narrow_S: workgroups per particle, from the full data set's tile count whatever the window."""
    tiles, E = (int(N_full) + 15) // 16, max(int(E), 1)
    if th >= 3:
        return max(1, min(64, n_cu // E, max(1, tiles // NRW_MAXW)))
    waves_per_particle = max(1, min(tiles, (16 * n_cu + E - 1) // E))
    return max(1, min(64, (waves_per_particle + NRW_MAXW - 1) // NRW_MAXW))


def waves(th, S, rows):
    """Waves per workgroup for `rows` rows (the full set's, or a window's count): narrow_waves, NRW_MAXW in the LDS form."""
    if th >= 3:
        return NRW_MAXW
    return max(1, min(NRW_MAXW, ((int(rows) + 15) // 16 + S - 1) // S))


def rows_per(rows, S):
    return ((int(rows) + S - 1) // S + 15) // 16 * 16


def walk(rows, S, nw):
    """[workgroup][wave] -> [(r0, valid rows)] of the tiles it takes."""
    rp = rows_per(rows, S)
    out = []
    for s in range(S):
        r_begin, r_end = s * rp, min(rows, s * rp + rp)
        out.append([[(r0, min(16, r_end - r0)) for r0 in range(r_begin + 16 * w, r_end, 16 * nw)] for w in range(nw)])
    return out


Launch = namedtuple('Launch', 'S nw rows walk')


def launch(inst, N_full, E, count=0):
    """The launch on `count` rows of a set of N_full (count 0: all of them)."""
    rows = count or N_full
    S = splits(N_full, E, inst[1])
    nw = waves(inst[1], S, rows)
    return Launch(S, nw, rows, walk(rows, S, nw))


def tile_counts(lch):
    """[workgroup] -> tiles of each wave."""
    return [[len(t) for t in wg] for wg in lch.walk]


def last_tile(lch):
    return max(t for wg in lch.walk for wv in wg for t in wv)


def cells(lch):
    out = {('waves', lch.nw)}
    for wg in tile_counts(lch):
        if sum(wg) == 0:
            out.add(('empty',))
        else:
            out |= {('tiles', min(n, 2)) for n in wg}
    valid = last_tile(lch)[1]
    out.add(('last', {16: 'full', 1: 'r1', 15: 'r15'}.get(valid, f'r{valid}')))
    return out


_WALK_CELLS = [('tiles', n) for n in (0, 1, 2)] + [('last', r) for r in ('full', 'r1', 'r15')]
CELLS = {'reg': [('waves', n) for n in (1, 2, 3, 4)] + _WALK_CELLS, 'lds': [('waves', 4)] + _WALK_CELLS}
# in a one-workgroup launch; a register form's idle wave needs a second workgroup (nw = min(4, tiles) at S = 1)
CELLS_ALONE = {'reg': [c for c in CELLS['reg'] if c != ('tiles', 0)], 'lds': CELLS['lds']}

# (N, E), smallest first.  Register forms: one workgroup of 1, 1, 2, 3, 4 waves and one tile each (last tile 1 row, full, 15 rows,
# 1 row, full); 80: workgroups of 3 and 2 tiles at three waves, one idle; 130: three workgroups of three; (200, 512): S = 2, waves
# of 2, 2, 2, 1 and 2, 2, 1, 1 tiles; (150, 2048): S = 1, 3, 3, 2, 2.  LDS forms: four waves always -- three idle, two idle with a
# 15-row tile, one tile each, 2, 2, 2, 1 in one workgroup, S = 2, and n_cu / E = 0.
FULL_CASES = {
    'reg': [(1, 2), (16, 2), (31, 2), (33, 2), (64, 2), (80, 2), (130, 2), (200, 512), (150, 2048)],
    'lds': [(1, 2), (31, 2), (64, 2), (100, 2), (128, 2), (64, 300)],
}
FULL_TILES = {      # (N, E) -> tiles of every wave of every workgroup
    'reg': {(1, 2): [[1]], (16, 2): [[1]], (31, 2): [[1, 1]], (33, 2): [[1, 1, 1]], (64, 2): [[1, 1, 1, 1]],
            (80, 2): [[1, 1, 1], [1, 1, 0]], (130, 2): [[1, 1, 1]] * 3, (200, 512): [[2, 2, 2, 1], [2, 2, 1, 1]],
            (150, 2048): [[3, 3, 2, 2]]},
    'lds': {(1, 2): [[1, 0, 0, 0]], (31, 2): [[1, 1, 0, 0]], (64, 2): [[1, 1, 1, 1]], (100, 2): [[2, 2, 2, 1]],
            (128, 2): [[1, 1, 1, 1]] * 2, (64, 300): [[1, 1, 1, 1]]},
}
# (begin, count) on N = 200, E = 2 (S = 4 for the register forms, 3 for the LDS forms); no begin is a multiple of 16, (177, 23) ends
# at the last row.  (45, 96) has an empty workgroup at S = 4 but neither that nor a ragged tile at S = 3, so the LDS forms also
# take (45, 90), whose 10-row last tile is followed by the data's rows 135 .. 140.
WINDOW_N, WINDOW_E = 200, 2
WINDOW_CASES = {'reg': [(13, 7), (13, 40), (45, 96), (177, 23)], 'lds': [(13, 7), (13, 40), (45, 96), (45, 90), (177, 23)]}
WINDOW_TILES = {
    'reg': {(13, 7): [[1], [0], [0], [0]], (13, 40): [[1], [1], [1], [0]], (45, 96): [[1, 1]] * 3 + [[0, 0]],
            (177, 23): [[1], [1], [0], [0]]},
    'lds': {(13, 7): [[1, 0, 0, 0]] + [[0] * 4] * 2, (13, 40): [[1, 0, 0, 0]] * 3, (45, 96): [[1, 1, 0, 0]] * 3,
            (45, 90): [[1, 1, 0, 0]] * 3, (177, 23): [[1, 0, 0, 0]] * 2 + [[0] * 4]},
}
MASK_ROWS = 64                  # the mask and head mutants are asked of the cases with at least this many rows


def case_id(case):
    return f'N{case[0]}-E{case[1]}'


def window_id(win):
    return f'rows{win[0]}+{win[1]}'


# ---- one net per instantiation ------------------------------------------------------------------------------------------------

Form = namedtuple('Form', 'inst part F hs act task')

ACTS = ('relu', 'tanh', 'sigmoid')
HIDDEN = {
    (1, 1, 1): (15,), (1, 1, 4): (16,), (1, 2, 1): (17,), (1, 2, 4): (31,),
    (2, 1, 1): (16, 15), (2, 1, 4): (9, 16), (2, 2, 1): (32, 15), (2, 2, 4): (17, 32),
    (3, 1, 1): (9, 16, 1), (3, 1, 4): (16, 15, 16), (3, 2, 1): (17, 9, 32), (3, 2, 4): (31, 16, 17),
    (1, 3, 1): (33,), (1, 3, 4): (48,), (1, 4, 1): (49,), (1, 4, 4): (64,),
    (2, 3, 1): (47, 33), (2, 3, 4): (33, 48), (2, 4, 1): (64, 49), (2, 4, 4): (63, 64),
    (3, 3, 1): (33, 48, 5), (3, 3, 4): (48, 17, 33), (3, 4, 1): (64, 49, 33), (3, 4, 4): (49, 64, 63),
}
DEEP = (16, 15, 9, 16, 12, 16, 15, 16, 7, 16)
F_OF = {1: (1, 5, 15, 16), 4: (17, 33, 60, 64)}
K_OF = (2, 5, 16)


def form_class(inst):
    return 'lds' if inst[1] >= 3 else ('deep' if inst[0] >= 4 else 'reg')


def walk_class(form):
    return 'lds' if weights_in_lds(form.inst) else 'reg'


def _forms():
    out = []
    for part, insts in ((False, FULL_INSTANTIATIONS), (True, PART_INSTANTIATIONS)):
        n_class, n_tf, n_k = {}, {1: int(part), 4: int(part)}, int(part)
        for inst in insts:
            nh, th, tf = inst
            cls = form_class(inst)
            i = n_class.get(cls, int(part))
            n_class[cls] = i + 1
            hidden = HIDDEN[inst] if nh <= 3 else ((15, 16, 1, 16, 15) if nh == 5 else DEEP[:nh])
            if part:
                hidden = hidden[::-1]           # the same widths, another layer the widest
            task = 'regr' if i % 2 == 0 else 'classification'
            K = 2
            if task == 'classification':
                K = K_OF[n_k % 3]
                n_k += 1
            F = F_OF[tf][n_tf[tf] % 4]
            n_tf[tf] += 1
            out.append(Form(inst, part, F, tuple(hidden) + (K,), ACTS[i % 3], task))
    return out


FORMS = _forms()


def form_id(form):
    return 'NH%d-TH%d-TF%d' % form.inst + ('-part' if form.part else '')


def form_name(form):
    return 'k_grad_narrow<%d,%d,%d%s>' % (form.inst + (',partition' if form.part else '',))


def full_cases(form):
    return FULL_CASES[walk_class(form)]


def window_cases(form):
    return WINDOW_CASES[walk_class(form)]


def data_sizes(form):
    """The sizes of the data sets the form's cases install, the window set's last."""
    return sorted({N for N, _ in full_cases(form)} - {WINDOW_N}) + [WINDOW_N]


def launches_on(form, N):
    """[(tag, begin, Launch)] of every launch the table makes on the data set of N rows."""
    out = [(case_id(c), 0, launch(form.inst, *c)) for c in full_cases(form) if c[0] == N]
    if N == WINDOW_N:
        out.append((case_id((WINDOW_N, WINDOW_E)), 0, launch(form.inst, WINDOW_N, WINDOW_E)))
        out += [(window_id(w), w[0], launch(form.inst, WINDOW_N, WINDOW_E, w[1])) for w in window_cases(form)]
    return out


# ---- problems -----------------------------------------------------------------------------------------------------------------

PRIOR_SCALE = 1000.0            # leaf_cases.ATTN_PRIOR_SCALE: the prior's gradient is -theta * 1e-6
KINK = 3e-7                     # of the layer's largest |z|: tests/test_gpu_parity.py's figure for "within fp32 rounding of the kink"
MIN_DRAW = 32                   # rows drawn for a smaller set (the oracle's regression targets are z-scored over the draw)
PAD_ROWS = 32                   # zero rows behind the data, as on the device
SEED_TRIES = 40
MUTANT_FACTOR = 10.0
# The GPU test holds the whole gradient to 2e-5 of its largest entry, the project's figure for fp32 accumulation over the rows.  A
# problem whose row sum cancels so far that the oracle itself, evaluated at float32, comes near that figure measures the problem:
# the float32 oracle must stay within a quarter of it.
WHOLE_F32 = 5e-6
# Likewise per leaf.  A leaf's entry is a sum over the rows; summed at float32 in any order it carries up to 2^-24 of the sum of the
# terms' absolute values.  Where that sum exceeds the leaf's largest entry so far that this rounding alone reaches a quarter of
# LEAF_TOL = 5e-5, the leaf measures the cancellation, and the float32 oracle's own error (one draw of that rounding, for a bias of
# one unit a single number) does not bound it: largest absolute sum / largest entry of every leaf below 5e-5 / 4 * 2^24 = 209.
CANCEL_MAX = 5e-5 / 4 * 2 ** 24
# what `search` printed: the parameter scale per form (0.1 where nothing is listed) and the seed per (form, data set size) (0 likewise)
SCALES = {'NH9-TH1-TF1': 0.3, 'NH8-TH1-TF1-part': 0.2}
SEEDS = {
    ('NH1-TH2-TF1', 200): 1, ('NH3-TH2-TF1', 64): 2, ('NH3-TH2-TF1', 130): 1, ('NH6-TH1-TF1', 1): 3, ('NH7-TH1-TF1', 80): 1,
    ('NH10-TH1-TF1', 64): 3, ('NH10-TH1-TF1', 80): 1, ('NH10-TH1-TF1', 130): 3, ('NH10-TH1-TF1', 150): 1, ('NH10-TH1-TF1', 200): 1,
    ('NH1-TH4-TF1', 100): 1, ('NH2-TH4-TF1', 100): 1, ('NH2-TH4-TF4', 200): 1, ('NH3-TH1-TF1-part', 130): 1,
    ('NH3-TH1-TF1-part', 150): 1, ('NH3-TH1-TF1-part', 200): 2, ('NH3-TH2-TF1-part', 64): 2, ('NH3-TH2-TF1-part', 200): 2,
    ('NH6-TH1-TF1-part', 130): 1, ('NH8-TH1-TF1-part', 200): 1, ('NH9-TH1-TF1-part', 64): 1, ('NH3-TH4-TF1-part', 100): 1,
    ('NH3-TH3-TF4-part', 64): 1,
}


def scale_of(form):
    return SCALES.get(form_id(form), 0.1)


def seed_of(form, N):
    return SEEDS.get((form_id(form), N), 0)


def ospec_of(form):
    from oracle import mclmc_oracle as M
    return M.ModelSpec(form.F, form.hs, activation=form.act, task=form.task, prior='Normal', prior_scale=PRIOR_SCALE)


def leaves_of(form):
    from tests import leafcheck as L
    from tests import partition_ref as PR
    return PR.compact_leaves(ospec_of(form)) if form.part else L.fcn_leaves(ospec_of(form))


def kernel_leaves(form):
    """[(leaf index, in, out)] of the kernel leaves among leaves_of(form)."""
    from oracle import mclmc_oracle as M
    ents = M.param_slices(ospec_of(form))
    out = []
    for j, (name, _, _) in enumerate(leaves_of(form)):
        if name.endswith('.kernel'):
            ent = ents[int(name[len('layer'):-len('.kernel')])]
            out.append((j, ent['in'], ent['out']))
    return out


def _live(form, theta):
    """A ReLU net's hidden biases made positive: a unit that is off on every row has a zero gradient row and column, and a kernel
    that dropped that row or column (the mask mutants) would be right."""
    from oracle import mclmc_oracle as M
    if form.act != 'relu':
        return theta
    theta = theta.copy()
    for ent in M.param_slices(ospec_of(form))[:-1]:
        b0, b1 = ent['bias']
        theta[:, b0:b1] = np.abs(theta[:, b0:b1])
    return theta


@lru_cache(maxsize=None)
def draw(form, N, seed, scale):
    """{'X' [N + PAD_ROWS, F], 'y', 'theta' [2, d], 'compact' [2, d_s] or None}: two chains of oracle.synthetic_problem, the rows
    followed by PAD_ROWS rows of zeros; for a partition form theta holds the frozen rows and a second draw the sampled layers.
    Shared between tests: read-only."""
    from oracle import mclmc_oracle as M
    from tests import partition_ref as PR
    ospec = ospec_of(form)
    prob = M.synthetic_problem(ospec, max(N, MIN_DRAW), 2, seed=seed, theta_scale=scale)
    X = np.concatenate([prob['X'][:N], np.zeros((PAD_ROWS, form.F), np.float32)])
    y = np.concatenate([prob['y'][:N], np.zeros(PAD_ROWS, prob['y'].dtype)])
    theta, compact = _live(form, prob['theta0']), None
    if form.part:
        other = M.synthetic_problem(ospec, max(N, MIN_DRAW), 2, seed=seed + 100, theta_scale=scale)['theta0']
        compact = PR.partition(ospec, _live(form, other))
    for a in (X, y, theta) + ((compact,) if form.part else ()):
        a.setflags(write=False)
    return {'X': X, 'y': y, 'theta': theta, 'compact': compact}


def problem(form, N):
    return draw(form, N, seed_of(form, N), scale_of(form))


def point(form, prob, E=2):
    """What logpost_grad takes, [E, dim] float32: particle e is chain e % 2."""
    p = prob['compact'] if form.part else prob['theta']
    return np.ascontiguousarray(np.tile(p, ((E + 1) // 2, 1))[:E])


def frozen(prob, E=2):
    return np.ascontiguousarray(np.tile(prob['theta'], ((E + 1) // 2, 1))[:E])


def _head_without_group(out, y, group):
    """The softmax head without the classes 4 group .. 4 group + 3: they take no part in the maximum, the sum or d(out)."""
    K = out.shape[-1]
    keep = np.ones(K, bool)
    keep[4 * group:4 * group + 4] = False
    m = out[..., keep].max(axis=-1, keepdims=True)
    e = np.where(keep, np.exp(out - m), 0.0)
    lse = m + np.log(e.sum(axis=-1, keepdims=True))
    yi = np.broadcast_to(y.astype(np.int64)[None, :, None], out.shape[:2] + (1,))
    ll = (np.take_along_axis(out, yi, axis=-1) - lse)[..., 0]
    dout = -np.where(keep, np.exp(out - lse), 0.0)
    np.put_along_axis(dout, yi, np.take_along_axis(dout, yi, axis=-1) + np.where(keep[yi], 1.0, 0.0), axis=-1)
    return ll, dout


def evaluate(form, prob, rows, dtype=np.float64, drop_group=None):
    """(logp [2], g [2, dim], likelihood part of g, the sum over the rows of the absolute value of each row's term of that part) of the
    two chains over the rows `rows` (indices into the padded data, repeats
    allowed), everything in `dtype`: the oracle's forward pass, head and prior, and its backward pass restated so that a head
    mutant can be put in (test_narrow_schedule_host.py holds it to oracle.logpost_and_grad and tests/partition_ref.py)."""
    from oracle import mclmc_oracle as M
    from tests import partition_ref as PR
    ospec = ospec_of(form)
    rows = np.asarray(rows, dtype=np.int64)
    X = prob['X'][rows].astype(dtype)
    y = prob['y'][rows] if prob['y'].dtype.kind == 'i' else prob['y'][rows].astype(dtype)
    sampled = (prob['compact'] if form.part else prob['theta']).astype(dtype)
    th = PR.merge(ospec, sampled, prob['theta'].astype(dtype)) if form.part else sampled
    out, zs, hs = M.mlp_forward(ospec, th, X, keep=True)
    ll, dz = M.pointwise_loglik(ospec, out, y) if drop_group is None else _head_without_group(out, y, drop_group)
    g, gabs = np.zeros_like(th), np.zeros_like(th)
    ents, layers = M.param_slices(ospec), M.unravel(ospec, th)
    for li in range(len(layers) - 1, -1, -1):
        k0, k1 = ents[li]['kernel']
        g[:, k0:k1] = (np.swapaxes(hs[li], 1, 2) @ dz).reshape(2, -1)
        gabs[:, k0:k1] = (np.swapaxes(np.abs(hs[li]), 1, 2) @ np.abs(dz)).reshape(2, -1)      # |outer(h, dz)| = outer(|h|, |dz|)
        b0, b1 = ents[li]['bias']
        g[:, b0:b1] = dz.sum(axis=1)
        gabs[:, b0:b1] = np.abs(dz).sum(axis=1)
        if li > 0:
            dz = (dz @ np.swapaxes(layers[li][0], 1, 2)) * M._act_grad(ospec.activation, zs[li - 1], hs[li])
    if form.part:
        g, gabs = np.ascontiguousarray(g[:, PR.index(ospec)]), np.ascontiguousarray(gabs[:, PR.index(ospec)])
    lp, gp = M.log_prior(ospec, sampled)
    return (lp + ll.sum(axis=-1)).astype(dtype), (g + gp).astype(dtype), g.astype(dtype), gabs.astype(dtype)


@lru_cache(maxsize=None)
def _reference(form, N, seed, scale, begin, count):
    from tests import leafcheck as L
    prob = draw(form, N, seed, scale)
    rows = np.arange(begin, begin + (count or N))
    lp, g, gl, gabs = evaluate(form, prob, rows)
    g32 = evaluate(form, prob, rows, np.float32)[1]
    assert g.dtype == np.float64 and g32.dtype == np.float32
    bound = L.leaf_bounds(leaves_of(form), 2, g32=g32, g_ref=g, tol=L.LEAF_TOL, margin=L.F32_MARGIN)
    for a in (lp, g, gl, g32, bound, gabs):
        a.setflags(write=False)
    return lp, g, gl, g32, bound, gabs


def reference(form, N, begin=0, count=0):
    """(logp [2], g [2, dim], its likelihood part, g of the same restatement at float32, the per-leaf bound [2, leaves], the rows'
    absolute sum of `evaluate`) on rows
    [begin, begin + count) of the tabulated problem of N rows (count 0: all).  Shared between tests: read-only."""
    return _reference(form, N, seed_of(form, N), scale_of(form), begin, count)


def near_kink(form, prob, N):
    """Hidden pre-activations of a ReLU net within KINK of their layer's largest, over the N rows of the data."""
    from oracle import mclmc_oracle as M
    from tests import partition_ref as PR
    if form.act != 'relu':
        return 0
    ospec = ospec_of(form)
    th = prob['theta'].astype(np.float64)
    if form.part:
        th = PR.merge(ospec, prob['compact'].astype(np.float64), th)
    _, zs, _ = M.mlp_forward(ospec, th, prob['X'][:N], keep=True)
    return int(sum((np.abs(z) < KINK * max(np.abs(z).max(), 1e-30)).sum() for z in zs[:-1]))


# ---- mutants ------------------------------------------------------------------------------------------------------------------

def _nonempty(lch):
    return [wg for wg in lch.walk if any(wg)]


def walk_mutants(lch, begin):
    """{name: rows} of what a wrong walk would sum, as indices into the padded data: the last tile of the first and of the last
    workgroup with a tile dropped, the rows behind a ragged last tile counted (under a window the data's next rows), wave 1 of the
    first workgroup and the last busy wave of the last one left out of the reduction."""
    def rows_of(tiles):
        return np.concatenate([np.arange(begin + r0, begin + r0 + v) for r0, v in tiles]) if tiles else np.zeros(0, np.int64)
    rows = np.arange(begin, begin + lch.rows)
    out = {}
    wgs = _nonempty(lch)
    for tag, wg in (('first', wgs[0]), ('last', wgs[-1])):
        out[f'last-tile-of-{tag}-workgroup-dropped'] = np.setdiff1d(rows, rows_of([max(t for wv in wg for t in wv)]))
    r0, valid = last_tile(lch)
    if valid < 16:
        out['trailing-rows-counted'] = np.concatenate([rows, np.arange(begin + r0 + valid, begin + r0 + 16)])
    if len(wgs[0]) > 1 and wgs[0][1]:
        out['wave-1-left-out'] = np.setdiff1d(rows, rows_of(wgs[0][1]))
    busy = [w for w in range(1, len(wgs[-1])) if wgs[-1][w]]
    if busy:
        out['last-busy-wave-left-out'] = np.setdiff1d(rows, rows_of(wgs[-1][busy[-1]]))
    return out


MASK_EDGES = (15, 16, 31, 32, 47, 48, 63)         # 16 k - 1 and 16 k


def mask_mutants(form, g, bound):
    """{name: least miss over the two chains} of a kernel leaf's gradient with input row or output column 16 k - 1 or 16 k zeroed,
    as a multiple of the leaf's bound: the row's or column's largest entry over the leaf's."""
    leaves = leaves_of(form)
    out = {}
    for j, n_in, n_out in kernel_leaves(form):
        name, b, e = leaves[j]
        G = np.abs(g[:, b:e]).reshape(2, n_in, n_out)
        top = G.max(axis=(1, 2))
        for k in MASK_EDGES:
            if k < n_in:
                out[f'{name}-row-{k}-zeroed'] = float((G[:, k, :].max(axis=1) / top / bound[:, j]).min())
            if k < n_out:
                out[f'{name}-column-{k}-zeroed'] = float((G[:, :, k].max(axis=1) / top / bound[:, j]).min())
    return out


def head_groups(form):
    """The lane groups whose classes the head mutant can drop and leave a class over."""
    K = form.hs[-1]
    return [] if form.task == 'regr' else [q for q in range((K + 3) // 4) if K > 4]


def mutant_misses(form, N, seed=None, scale=None):
    """{(launch tag, mutant name): least miss of the per-leaf bound over the two chains, as a multiple of the bound} over every
    launch the table makes on the data set of N rows."""
    from tests import leafcheck as L
    seed = seed_of(form, N) if seed is None else seed
    scale = scale_of(form) if scale is None else scale
    prob, leaves = draw(form, N, seed, scale), leaves_of(form)
    out = {}
    for tag, begin, lch in launches_on(form, N):
        _, g, _, _, bound, _ = _reference(form, N, seed, scale, begin, 0 if lch.rows == N else lch.rows)
        for name, rows in walk_mutants(lch, begin).items():
            g_mut = evaluate(form, prob, rows)[1]
            out[(tag, name)] = float((L.leaf_errors(g_mut, g, leaves) / bound).max(axis=1).min())
        if lch.rows >= MASK_ROWS:
            for name, miss in mask_mutants(form, g, bound).items():
                out[(tag, name)] = miss
            for q in head_groups(form):
                g_mut = evaluate(form, prob, np.arange(begin, begin + lch.rows), drop_group=q)[1]
                out[(tag, f'classes-of-lane-group-{q}-dropped')] = float((L.leaf_errors(g_mut, g, leaves) / bound).max(axis=1).min())
    return out


def audit(form, N, seed=None, scale=None):
    """(pre-activations near the kink, least likelihood share, float32 oracle's worst leaf as a multiple of its bound, float32
    oracle's whole-gradient error, worst cancellation of a leaf, least mutant miss and its name) of the data set of N rows: what `search` and the host test ask
    of a tabulated problem."""
    from tests import leafcheck as L
    seed = seed_of(form, N) if seed is None else seed
    scale = scale_of(form) if scale is None else scale
    prob, leaves = draw(form, N, seed, scale), leaves_of(form)
    share, f32, whole32, cancel = np.inf, 0.0, 0.0, 0.0
    for _, begin, lch in launches_on(form, N):
        _, g, gl, g32, bound, gabs = _reference(form, N, seed, scale, begin, 0 if lch.rows == N else lch.rows)
        cancel = max(cancel, float(max((gabs[:, b:e].max(axis=1) / np.abs(g[:, b:e]).max(axis=1)).max() for _, b, e in leaves)))
        share = min(share, float(L.likelihood_share(gl, g, leaves).min()))
        f32 = max(f32, float((L.leaf_errors(g32, g, leaves) / bound).max()))
        whole32 = max(whole32, float((np.abs(g32 - g).max(axis=1) / np.abs(g).max(axis=1)).max()))
    misses = mutant_misses(form, N, seed, scale)
    worst = min(misses, key=misses.get)
    return near_kink(form, prob, N), share, f32, whole32, cancel, misses[worst], worst


def clean(form, N, seed, scale):
    from tests import leaf_cases as LC
    kink, share, f32, whole32, cancel, miss, _ = audit(form, N, seed, scale)
    return kink == 0 and share >= LC.MIN_SHARE and f32 < 1.0 and whole32 < WHOLE_F32 and cancel < CANCEL_MAX and miss > MUTANT_FACTOR


def search(forms=None):
    """Prints SCALES and SEEDS: per form the first scale of leaf_cases.THETA_LADDER at which every data set has a clean seed, and
    per data set the first such seed."""
    from tests import leaf_cases as LC
    scales, seeds = {}, {}
    for form in forms or FORMS:
        for scale in LC.THETA_LADDER:
            found = {}
            for N in data_sizes(form):
                seed = next((sd for sd in range(SEED_TRIES) if clean(form, N, sd, scale)), None)
                if seed is None:
                    break
                found[N] = seed
            _reference.cache_clear()
            draw.cache_clear()
            if len(found) == len(data_sizes(form)):
                break
        else:
            raise AssertionError(f'no scale of the ladder gives every data set of {form_id(form)} a clean seed')
        if scale != 0.1:
            scales[form_id(form)] = scale
        seeds.update({(form_id(form), N): sd for N, sd in found.items() if sd})
        print(f'# {form_id(form)}: scale {scale}, seeds {found}', flush=True)
    print('SCALES =', scales)
    print('SEEDS =', seeds)


if __name__ == '__main__':
    search()

"""The case table of tests/attn_schedule.py has no holes, proven without a GPU: the restatement's constants and formulas are the
sources' and the specs', every cell of the three attention kernels' schedule that can be reached gets a launch and what cannot is
proven so by enumeration, no case is there for nothing, every case keeps every leaf's likelihood share at 0.5 or more and its
attention sharp (with the exceptions attn_schedule.py states and this file proves), and a schedule that is wrong in one of the ways
below misses the per-leaf bound of tests/test_gpu_attn_schedule.py by 10x or more on a leaf it touches, on every case that has the
property.  The factors found are printed (ATTNSCHED lines); profiles/r11/01_attn_schedule.md keeps them.

The mutants are built on a second fp64 restatement (torch autograd, `_model` below), which is first held to tests/attn_ref.py /
tests/attn_pre_ref.py leaf by leaf at 1e-9; the ones that are sums over rows or over two calls are built from the per-sequence
gradients of the NumPy restatement."""
import math
import re
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

from tests import attn_schedule as S
from tests import leafcheck as L

CSRC = Path(__file__).resolve().parents[1] / 'mile_amd' / 'csrc'
TABLE = 'TokenEmbedding_0.Embedding.embedding'
POS = 'TokenEmbedding_0.PositionEmbedding.embedding'


# ---- the restatement against the sources -------------------------------------------------------------------------------------------

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


def _define(text, name):
    m = re.findall(r'#define ' + name + r'\s+\(?([0-9* ]+)\)?', text)
    assert len(m) == 1, (name, m)
    return eval(m[0])                                             # digits, '*' and blanks only


def test_constants_are_the_sources():
    """Each constant and formula where its function states it: a later change fails here instead of silently emptying a cell."""
    attn, pre, wide, hip = _src('mile_attn.h'), _src('mile_attn_pre.h'), _src('mile_attn_wide.h'), _src('mile_hip.hip')
    assert _define(attn, 'ATTN_NT') == S.NT and _define(attn, 'ATTN_MAX_T') == S.MAX_T and _define(attn, 'ATTN_MAX_K') == S.MAX_K
    assert _define(attn, 'ATTN_MAX_NP') == S.MAX_NP and _define(attn, 'ATTN_LDS_MAX') == S.LDS_MAX == 160 * 1024
    assert {k: _define(attn, 'ATTN_MAX_' + k) for k in 'CDP'} == S.LIMITS['attn']
    assert {k: _define(pre, 'ATTNP_MAX_' + k) for k in 'CDP'} == S.LIMITS['pre'] == S.LIMITS['wide']
    assert _define(hip, 'ATTN_WIDE_MIN_ROWS') == S.WIDE_MIN_ROWS
    b = _body(hip, 'attn_ranges')
    assert f'std::min({{{S.RANGE_CAP}, want, std::max(1, rows / {S.RANGE_MIN_ROWS})}})' in b and 'const int want = (n_cu + std::max(E, 1) - 1) / std::max(E, 1);' in b
    assert 'return std::max(1, std::min(want, std::max(1, rows / ATTN_WIDE_MIN_ROWS)));' in _body(hip, 'attn_wide_S_rows')
    assert 'return attn_ranges(s->n_cu, E, s->N);' in _body(hip, 'attn_S') and 's->win_count ? s->win_count : s->N' in _body(hip, 'attn_wide_S')
    b = _body(attn, 'attn_body')
    assert f'constexpr int NJ = ATTN_MAX_T / 16, NDW = {S.NDW}, NDP = {S.NDP}, NFW = ATTN_MAX_P / 4;' in b and S.NFW == S.LIMITS['attn']['P'] // 4
    assert 4 * S.NDW == 4 * 3 * 4 and 4 * S.NDP == (S.MAX_T // 16) * 4                      # the register arrays hold the most tiles of the envelope
    for body in (b, _body(pre, 'attnp_body')):
        assert 'const int rows_per = (p.N + nsplit - 1) / nsplit;' in body and 'for (int h = wave; h < H; h += 4)' in body
        assert 'const int r_begin = min(p.N, s * rows_per), r_end = min(p.N, r_begin + rows_per);' in body
        assert 'nj = Tp / 16, CT = (C + 15) / 16, ND = (D + 15) / 16;' in body
    assert 'for (int f = wave; f < nj * 3 * ND; f += 4)' in b and 'if (f < CT * 3 * ND)' in b and 'if (f < nj * CT)' in b
    pb = _body(pre, 'attnp_body')
    assert 'for (int f = wave; f < 3 * ND; f += 4)' in pb and 'for (int f = wave; f < CT * 3 * ND; f += 4)' in pb
    assert 'for (int ct = wave; WIDE && ct < CT; ct += 4)' in pb and 'const bool first = row == r_begin;' in pb
    assert 'const int dr = ATTN_NT / nb, dc = ATTN_NT - dr * nb;' in pb
    assert 'const int n = V * C, head = min(n, (4 - (g.emb & 3)) & 3), nq = (n - head) >> 2;' in pb
    assert 'return 5 * Tp + 10 * 64 + 16;' in _body(attn, 'attn_vec_floats')
    assert 'return 16 * g.Tp + (g.hd > 16 ? g.Tp * ((g.hd + 15) / 16 * 16) : 0);' in _body(attn, 'attn_scr_wave')
    assert 'const int w = g.H < 4 ? g.H : 4, a = 64 * g.Tp, b = w * attn_scr_wave(g);' in _body(attn, 'attn_scr_floats')
    assert 'return ((size_t)(wl ? g.C * 3 * g.D : 0) + (size_t)g.Tp * 3 * g.D + attn_scr_floats(g) + attn_vec_floats(g.Tp)) * 4;' in _body(attn, 'attn_lds_bytes')
    assert 'return attn_lds_bytes(g, true) <= ATTN_LDS_MAX;' in _body(attn, 'attn_weights_in_lds')
    assert 'return attn_lds_bytes(g, false) <= ATTN_LDS_MAX;' in _body(attn, 'attn_supported')
    assert 'return 17 * g.Tp + (g.hd > 16 ? g.Tp * ((g.hd + 15) / 16 * 16) : 0);' in _body(pre, 'attnp_scr_wave')
    assert 'const int w = g.H < 4 ? g.H : 4, a = g.Tp * g.C, b = w * attnp_scr_wave(g);' in _body(pre, 'attnp_scr_floats')
    assert 'return ((size_t)g.Tp * 3 * g.D + attnp_scr_floats(g) + attnp_vec(g).n) * 4;' in _body(pre, 'attnp_lds_bytes')
    assert 'return attnp_lds_bytes(g) <= ATTN_LDS_MAX;' in _body(pre, 'attnp_supported') and 'return attnp_supported(g)' in _body(wide, 'attn_wide_supported')
    assert 'if ((p.g.hd + 15) / 16 != NHT)' in _body(attn, 'attn_launch')
    launch = _src('mile_attn.hip')
    assert 'attn_launch<AttnKernels<true>, 4>' in launch and S.MAX_NHT['attn'] == 4
    for f, name in (('pre', 'mile_attn_pre.hip'), ('wide', 'mile_attn_wide.hip')):
        assert re.search(r'attn_launch<\w+, 8>', _src(name)) and S.MAX_NHT[f] == 8, name
    for f in S.FAMILIES:
        assert S.REFUSAL[f].split(': ')[1] in _body(hip, 'layout_attn_model') and f'"{S.REFUSAL[f].split(":")[0]}"' in hip, f
    assert S.LIMIT_REFUSAL['attn'].split(': ')[1].replace('64', '') == 'qkv_dim <=  and n_heads dividing it' and '": qkv_dim <= "' in hip


@pytest.mark.parametrize('case', [c for c in S.CASES if c.prev is None], ids=lambda c: c.name)
def test_plan_is_the_specs_and_the_librarys(case):
    """The LDS size is spec.lds_bytes, the restated S is WideAttentionSpec.row_splits, the offsets are spec.leaves()', and the
    library makes an engine of the geometry (mile_create needs no GPU)."""
    spec = S.spec_of(case)
    assert S.supported(case) and S.lds_bytes(case) == spec.lds_bytes <= S.LDS_MAX
    if case.family == 'wide':
        assert S.launch(case)['S'] == spec.row_splits(case.E, case.N)
    off, leaves = S.offsets(case), {n: o for n, o, _ in spec.leaves()}
    assert off['d'] == spec.n_params and off['k_q'] == leaves['MDPA.query.kernel'] and off['k_c'] == leaves['classifier.kernel']
    assert off['emb'] == leaves.get(TABLE, -1) and off['b_v'] == leaves.get('MDPA.value.bias', -1)
    rc, msg, _ = S.library_refuses(case.family, case.V, case.T, case.C, case.H, case.D, case.K, case.proj, case.bias)
    assert rc == 0, (case.name, msg)


def test_known_figures():
    """What the issue and the sources state, from the restatement."""
    assert S.launch(S.BY_NAME['attn-rows289'])['counts'] == [17] * 17 + [0] and S.attn_ranges(256, 14, 289) == 18 and S.attn_ranges(256, 15, 289) == 18
    assert S.launch(S.BY_NAME['wide-rows81'])['counts'] == [9] * 9 + [0] and S.attn_wide_S_rows(256, 25, 81) == 10 and S.attn_wide_S_rows(256, 29, 81) == 9
    assert S.launch(S.BY_NAME['pre-rows273'])['counts'][-1] == 1 and S.launch(S.BY_NAME['wide-rows74-e1'])['counts'][-1] == 2
    assert S.launch(S.BY_NAME['attn-seq-win3'])['counts'] == [1, 1, 1] + [0] * 7 and S.launch(S.BY_NAME['wide-seq-win3'])['S'] == 1
    assert S.launch(S.BY_NAME['wide-seq-win37'])['counts'] == [10, 10, 10, 7] and S.launch(S.BY_NAME['wide-seq-full'])['S'] == 20
    assert S.attn_wide_S_rows(256, 1, 35000) == 256 and S.attn_wide_S_rows(256, 1, 256) == 32 and S.attn_ranges(256, 1, 35000) == 64
    assert S.head_owner(5) == {0: [0, 4], 1: [1], 2: [2], 3: [3]} and S.head_owner(12)[3] == [3, 7, 11]
    assert S.attn_lds_bytes(70, 48, 8, 64, True) == S.spec_of(S._c('x', 'attn', 1000, 70, 48, 8, 64)).lds_bytes
    assert S.zero_fill(S.BY_NAME['wide-seq-full']) == (1, 3, 1574, 1) and S.zero_fill(S.BY_NAME['wide-c2-d4-bias'])[:2] == (1, 2)
    assert {S.zero_fill(c)[0] for c in S.CASES if c.family == 'wide'} == {0, 1, 2, 3} == {S.zero_fill(c)[3] for c in S.CASES if c.family == 'wide'}
    assert S.rank1_calls(S.BY_NAME['pre-hd5-h3']) == [('classifier.kernel', 5, 3, 85, 1), ('projection_1.kernel', 6, 5, 51, 1),
                                                    ('projection_0.kernel', 10, 6, 42, 4), ('MDPA.out.kernel', 15, 10, 25, 6)]
    assert S.tile_loops(S.BY_NAME['attn-most-tiles']) == {'qkv': 96, 'dW': 48, 'de': 32} == S.LOOP_MOST


# ---- coverage ------------------------------------------------------------------------------------------------------------------------

def _divisors(D):
    return [h for h in range(1, D + 1) if D % h == 0]


def test_every_cell_gets_a_launch(capsys):
    hit = {}
    for c in S.CASES:
        for cell in S.cells_of(c):
            hit.setdefault(cell, []).append(c.name)
    for c in S.EVAL_CASES:
        for cell in S.eval_cells_of(c):
            hit.setdefault(cell, []).append(c.name)
    assert set(hit) <= set(S.CELLS), sorted(set(hit) - set(S.CELLS), key=str)               # nothing runs outside the enumeration
    assert set(S.UNREACHABLE) <= set(S.CELLS) and not set(S.UNREACHABLE) & set(hit)
    missing = [cell for cell in S.CELLS if cell not in hit and cell not in S.UNREACHABLE]
    assert not missing, missing
    assert all(S.supported(c) for c in S.CASES)                                             # and nothing is launched outside the envelope
    with capsys.disabled():
        fam = {}
        for cell in S.CELLS:
            fam[cell[0]] = fam.get(cell[0], 0) + 1
        print(f'\nATTNSCHED {len(S.CELLS)} cells, {len(S.UNREACHABLE)} unreachable, {len(S.CASES)} cases, {len(S.EVAL_CASES)} of them evaluated; '
              'per kind: ' + ', '.join(f'{k} {v}' for k, v in fam.items()))


def test_no_case_is_there_for_nothing():
    """Every case has a cell that no case before it in the table has; the four gradients of a window sequence count as one."""
    seen, seq = set(), {n for names in S.SEQUENCES.values() for n in names}
    for c in S.CASES:
        if c.name in seq:
            continue
        cells = S.cells_of(c) | (S.eval_cells_of(c) if c in S.EVAL_CASES else set())
        assert cells - seen, c.name
        seen |= cells
    for f, names in S.SEQUENCES.items():
        cells = set().union(*(S.cells_of(S.BY_NAME[n]) for n in names))
        assert {('window', f, w) for w in S.WINDOWS} <= cells - seen, f
    keys = [c[1:] for c in S.CASES]
    assert len(set(keys)) == len(keys)


def test_unreachable_cells_by_enumeration():
    """The whole on-chip envelope (T enters through Tp alone): NHT = 3 never streams its weights, the other three do somewhere;
    two heads on a wave never meet dK in scratch; a q | k | v tile count is never one round.  Both bounds of 160 KiB: the recorded
    geometries are the largest next to a flip or a refusal, and sit on or just under the bound."""
    wl = {}
    most = {'wl': (0, None), 'attn': (0, None)}
    for Tp in range(16, S.MAX_T + 1, 16):
        for D in range(1, S.LIMITS['attn']['D'] + 1):
            for H in _divisors(D):
                hd = D // H
                assert not (H > 4 and hd > 16)
                free = S.attn_lds_bytes(Tp, 1, H, D, False)                                  # C does not enter without the weights
                if free > S.LDS_MAX:
                    continue
                if Tp < S.MAX_T and S.attn_lds_bytes(Tp + 16, 1, H, D, False) > S.LDS_MAX and free > most['attn'][0]:
                    most['attn'] = (free, (Tp, H, D))
                for C in range(1, S.LIMITS['attn']['C'] + 1):
                    b = S.attn_lds_bytes(Tp, C, H, D, True)
                    wl.setdefault((hd + 15) // 16, set()).add(b <= S.LDS_MAX)
                    if b <= S.LDS_MAX and Tp < S.MAX_T and S.attn_supported(Tp + 16, C, H, D) and not S.attn_weights_in_lds(Tp + 16, C, H, D) \
                            and b > most['wl'][0]:
                        most['wl'] = (b, (Tp, C, H, D))
    assert wl == {1: {True, False}, 2: {True, False}, 3: {True}, 4: {True, False}}
    assert S.attn_lds_bytes(128, 64, 1, 48, True) == 148544                                  # the corner the proof in UNREACHABLE names
    assert most['wl'][0] == S.LDS_MAX == S.attn_lds_bytes(*S.BOUND_WL, True) and S.attn_lds_bytes(S.BOUND_WL[0] + 16, *S.BOUND_WL[1:], True) == 182592
    assert most['attn'][0] == 154048 == S.attn_lds_bytes(*S.BOUND_ATTN[:4], False) and S.attn_lds_bytes(S.BOUND_ATTN[0] + 16, *S.BOUND_ATTN[1:4], False) == 175680
    best = (0, None)
    for Tp in range(16, S.MAX_T, 16):
        for D in range(1, S.LIMITS['pre']['D'] + 1):
            for H in _divisors(D):
                Cs = np.arange(1, S.LIMITS['pre']['C'] + 1)
                hd = D // H
                scr = np.maximum(Tp * Cs, min(H, 4) * S.attnp_scr_wave(Tp, hd))
                scr2 = np.maximum((Tp + 16) * Cs, min(H, 4) * S.attnp_scr_wave(Tp + 16, hd))
                b = 4 * (Tp * 3 * D + scr + Tp + 2 * D + 4 * Cs + 16)                        # attnp_vec without projections: C + zf + 2 W = 4 C
                b2 = 4 * ((Tp + 16) * 3 * D + scr2 + Tp + 16 + 2 * D + 4 * Cs + 16)
                ok = (b <= S.LDS_MAX) & (b2 > S.LDS_MAX)
                if ok.any() and b[ok].max() > best[0]:
                    best = (int(b[ok].max()), (Tp, int(Cs[ok][b[ok].argmax()]), H, D))
    assert best[0] == S.LDS_MAX == S.attnp_lds_bytes(*S.BOUND_STREAMED[:4]) and S.attnp_lds_bytes(S.BOUND_STREAMED[0] + 16, *S.BOUND_STREAMED[1:4]) == 196416, best   # (ties: the recorded one is the first in T, C)
    for f, T, C, H, D, proj, K in S.REFUSED:
        sup = S.attn_supported if f == 'attn' else S.attnp_supported
        assert not sup(T, C, H, D, K, proj) and sup(T - 16, C, H, D, K, proj)
        rc, msg, _ = S.library_refuses(f, 60, T, C, H, D, K, proj)
        assert rc != 0 and msg == S.REFUSAL[f]
    (f, T, C, H, D, proj, K), = S.REFUSED_BY_LIMIT
    assert S.library_refuses(f, 25, T, C, H, D, K, proj)[1] == S.LIMIT_REFUSAL['attn']
    for f in S.FAMILIES:                                                                     # 3 divides the count, 4 does not divide 3 n
        assert all(n % 3 == 0 for c in S.CASES if c.family == f for k, n in S.tile_loops(c).items() if k != 'de')


# ---- the problems ------------------------------------------------------------------------------------------------------------------

def _names(P):
    return [n for n, _, _ in P.leaves]


@pytest.mark.parametrize('case', S.CASES, ids=lambda c: c.name)
def test_every_leaf_sees_the_likelihood_and_attention_is_sharp(case):
    """likelihood_share >= leaf_cases.MIN_SHARE on every leaf of both chains on the case's rows, but for the leaves whose
    likelihood gradient is zero analytically (attn_schedule.zero_leaves: they are asserted to be rounding) and for the Normal(0.2)
    case of each family; the thresholds of tests/test_leafcheck_host.py on attention_stats, but for the cases that are flat by
    construction.  A case with a recorded qk_scale misses a threshold at every scale before it in QK_LADDER."""
    from tests import leaf_cases as LC
    P = S.problem(case)
    _, g, g32 = S.reference_of(case)
    gl = P.lik(P.rows)
    zero = S.zero_leaves(case, _names(P))
    share = L.likelihood_share(gl, g, P.leaves)
    ref_scale = np.abs(gl).max()
    for j, (n, b, e) in enumerate(P.leaves):
        if n in zero:
            assert np.abs(gl[:, b:e]).max() <= 1e-12 * max(ref_scale, 1e-300), (case.name, n)
        elif not S.prior_dominated(case):
            assert share[:, j].min() >= LC.MIN_SHARE, (case.name, n, share[:, j])
    assert g32.dtype == np.float32 and np.isfinite(g32).all()

    def sharp(P):
        st = P.stats()
        return all(s['median_top'] >= 0.2 and s['min_rel'] <= 1e-6 and s['max_logit'] < 80.0 for s in st)

    if S.flat_by_construction(case):
        assert not sharp(P) or case.name == 'pre-c2-d4-bias'
    else:
        assert sharp(P), (case.name, P.stats())
    base = case.name if case.prev is None else S.SEQUENCES[case.family][0]
    if base in S.QK_SCALE and case.prev is None:
        for qk in S.QK_LADDER[:S.QK_LADDER.index(S.QK_SCALE[base])]:
            assert not sharp(S.problem(case, qk)), (case.name, qk)
    else:
        assert case.name not in S.QK_SCALE


def test_problem_tiles_two_chains():
    case = S.BY_NAME['wide-rows40-e128']
    P = S.problem(case)
    th = P.theta()
    assert th.shape == (128, P.spec.n_params) and th.dtype == np.float32 and np.array_equal(th[2], th[0]) and np.array_equal(th[127], th[1])
    assert not np.array_equal(th[0], th[1]) and P.spec.prior_scale == S.WIDE_PRIOR and S.spec_of(S.BY_NAME['pre-normal']).prior_scale == 0.2
    win = S.BY_NAME['attn-seq-win37']
    assert np.array_equal(S.rows_x(win), S.problem(win).prob['x'][20:57]) and S.problem(win).rows == slice(20, 57)
    lp, g, g32 = S.reference_of(win)
    assert lp.shape == (2,) and not g.flags.writeable and np.abs(g - S.reference_of(S.BY_NAME['attn-seq-full'])[1]).max() > 0


# ---- mutants -----------------------------------------------------------------------------------------------------------------------

def _model(case, P, chain, rows, mut=None):
    """log-likelihood of chain `chain` over `rows` in torch fp64 and its gradient by autograd -> (flat gradient, d(e) [n, T, C]).
    `mut`: 'hd-tail' (the last hd % 4 terms of every score dropped), 'c-tail' (the last C % 4 terms of q, k and v dropped),
    'pad-keys' (positions T..Tp, whose e is zero, taken as keys of the real query rows), 'second-head' (no backward through
    the heads >= 4: a wave's second and later ones), 'nht-cols' (no backward through the columns >= 16 of q and k of a head)."""
    import torch
    import torch.nn.functional as F
    spec, prob = P.spec, P.prob
    x = torch.from_numpy(np.array(prob['x'][rows], dtype=np.int64))
    y = torch.from_numpy(np.array(prob['y'][rows], dtype=np.int64))
    th = torch.tensor(prob['theta0'][chain].astype(np.float64), requires_grad=True)
    leaf = {n: th[o:o + int(np.prod(sh))].reshape(sh) for n, o, sh in spec.leaves()}
    n, T = x.shape
    C, H, D, b = case.C, case.H, case.D, case.bias
    hd = D // H
    if case.family == 'pre':
        emb, pos = torch.from_numpy(prob['emb'].astype(np.float64)), torch.from_numpy(prob['pos'].astype(np.float64))
    else:
        emb, pos = leaf[TABLE], leaf[POS]
    e = emb[x] + pos[None, :T]
    e.retain_grad() if e.requires_grad else None
    kc = C - C % 4 if mut == 'c-tail' else C
    proj = lambda name: (e[..., :kc] @ leaf[f'MDPA.{name}.kernel'].reshape(C, D)[:kc]) + (leaf[f'MDPA.{name}.bias'].reshape(D) if b else 0.0)   # noqa: E731
    q, k, v = proj('query'), proj('key'), proj('value')
    real = x != 0
    keym = real
    if mut == 'pad-keys':
        npad = S.up(T, 16) - T
        zero = torch.zeros(n, npad, D, dtype=torch.float64)
        k = torch.cat([k, zero + (leaf['MDPA.key.bias'].reshape(D) if b else 0.0)], dim=1)
        v = torch.cat([v, zero + (leaf['MDPA.value.bias'].reshape(D) if b else 0.0)], dim=1)
        keym = torch.cat([real, torch.ones(n, npad, dtype=torch.bool)], dim=1)
    heads = lambda t: t.reshape(n, t.shape[1], H, hd).transpose(1, 2)                        # noqa: E731
    qh, kh, vh = heads(q / math.sqrt(hd)), heads(k), heads(v)
    if mut == 'second-head':
        keep = (torch.arange(H) < 4).to(torch.float64)[None, :, None, None]
        for t in (qh, kh, vh):
            t.register_hook(lambda gr: gr * keep)
    if mut == 'nht-cols':
        keep = (torch.arange(hd) < 16).to(torch.float64)
        for t in (qh, kh):
            t.register_hook(lambda gr: gr * keep)
    m = hd - hd % 4 if mut == 'hd-tail' else hd
    s = qh[..., :m] @ kh[..., :m].transpose(2, 3)
    mask = (real[:, :, None] & keym[:, None, :])[:, None]
    s = torch.where(mask, s, torch.tensor(float(np.finfo(np.float32).min), dtype=torch.float64))
    if mut == 'pad-keys':                                           # a pad query row stays uniform over the T positions
        s = torch.cat([s[..., :T], torch.where(real[:, None, :, None], s[..., T:], torch.tensor(-math.inf, dtype=torch.float64))], dim=-1)
    p = torch.softmax(s, dim=-1)
    oc = (p @ vh).transpose(1, 2).reshape(n, T, D)
    z = (oc @ leaf['MDPA.out.kernel'].reshape(D, C) + (leaf['MDPA.out.bias'] if b else 0.0)).mean(dim=1)
    for i in range(len(case.proj)):
        z = F.gelu(z @ leaf[f'projection_{i}.kernel'] + (leaf[f'projection_{i}.bias'] if b else 0.0), approximate='tanh')
    if case.family == 'pre':
        z = F.gelu(z, approximate='tanh')
    lg = z @ leaf['classifier.kernel'] + (leaf['classifier.bias'] if b else 0.0)
    ll = torch.log_softmax(lg, dim=1)[torch.arange(n), y].sum()
    ll.backward()
    return th.grad.numpy().copy(), (e.grad.numpy().copy() if e.requires_grad else None)


@lru_cache(maxsize=None)
def _row_grads(key, qk):
    """The likelihood gradient of every single sequence of the case's whole data set: [2, N, d] (fp64, the NumPy restatement)."""
    case = S._c('rows', *key[:7], proj=key[7], bias=key[8], N=key[9], seed=key[10], prior_scale=key[11])
    P = S.problem(case, qk)
    return np.stack([np.stack([P.lik(slice(i, i + 1))[c] for i in range(case.N)]) for c in range(2)])


def _rows_lik(case):
    return _row_grads(S._key(case), S.qk_of(case))


def _slots(case):
    """What one gradient of `case` leaves in the slab rows: {e S + s: (chain, first row, last row + 1)} in the data set's rows."""
    b0, _ = S.rows_of(case)
    Lc = S.launch(case)
    return {e * Lc['S'] + s: (e % 2, b0 + b, b0 + en) for e in range(case.E) for s, (b, en) in enumerate(Lc['spans'])}


def schedule_mutants(case):
    """{name: (gradient [2, d], names of the leaves it may touch)} of what a wrong schedule would return for `case`; only what the
    case's schedule can get wrong.  The forms that need earlier calls read what the cases before it on the same engine (case.prev, and those before it) left."""
    P = S.problem(case)
    names = _names(P)
    span = {n: (b, e) for n, b, e in P.leaves}
    _, g, _ = S.reference_of(case)
    g = np.array(g)
    geo, Lc = S.geometry(case.T, case.C, case.H, case.D), S.launch(case)
    b0, nrows = S.rows_of(case)
    rows = slice(b0, b0 + nrows)
    zero = S.zero_leaves(case, names)
    every = [n for n in names if n not in zero]
    slab = [n for n in every if n != TABLE]                          # what a workgroup owns in its slab row without atomics
    streamed = case.family in S.STREAMED
    out = {}
    if case.K == 1:
        return out

    def only(leafnames, g_other):
        gm = g.copy()
        for n in leafnames:
            b, e = span[n]
            gm[:, b:e] = g_other[:, b:e]
        return gm

    def model(mut):
        gl = np.stack([_model(case, P, c, rows)[0] for c in range(2)])
        return g - gl + np.stack([_model(case, P, c, rows, mut)[0] for c in range(2)])

    G = None
    if nrows > 1 or case.prev is not None:
        G = _rows_lik(case)
    if nrows > 1:
        last = [b0 + e - 1 for b, e in Lc['spans'] if e > b]
        out['last-sequence-of-a-range-dropped'] = (g - G[:, last].sum(axis=1), every)
    if streamed and any(c >= 2 for c in Lc['counts']):
        firsts = [b0 + b for b, e in Lc['spans'] if e - b >= 2]
        out['second-sequence-stored'] = (only(slab, g - G[:, firsts].sum(axis=1)), slab)
    if case.H > 4:
        out['second-head-left-out'] = (model('second-head'), [n for n in every if n.startswith(('MDPA.query', 'MDPA.key', 'MDPA.value', 'Token'))])
    if geo['NHT'] > 1:
        out['dq-dK-columns-dropped'] = (model('nht-cols'), [n for n in every if n.startswith(('MDPA.query', 'MDPA.key'))])
    if geo['hd'] % 4 and geo['hd'] > 4 and case.T > 1:
        out['score-tail-dropped'] = (model('hd-tail'), every)
    if case.C % 4 and case.C > 4:
        out['C-tail-dropped'] = (model('c-tail'), every)
    if case.T % 16 and case.T > 1:
        out['pad-positions-as-keys'] = (model('pad-keys'), every)
    x = np.asarray(P.prob['x'][rows])
    if case.family != 'pre' and S.MASKS[4] in S.mask_kinds(x, case.V):
        gm = g.copy()
        b, e = span[TABLE]
        for c in range(2):
            gfull, de = _model(case, P, c, rows)
            summed, stored = np.zeros((case.V, case.C)), np.zeros((case.V, case.C))
            for i in range(x.shape[0]):
                one = np.zeros((case.V, case.C))
                for t in range(case.T):
                    one[x[i, t]] = de[i, t]                          # the later position overwrites the earlier one
                stored += one
                np.add.at(summed, x[i], de[i])
            assert np.abs(summed.reshape(-1) - gfull[b:e]).max() <= 1e-9 * np.abs(gfull[b:e]).max()
            gm[c, b:e] += (stored - summed).reshape(-1)
        out['duplicate-token-stored'] = (gm, [TABLE])
    if S.geometry(case.T, case.C, case.H, case.D)['hd'] > 1 and case.T > 1:
        for mut in ('dq_unscaled', 'ds_unmasked'):
            gm = P.ref(rows=rows, mutant=mut)[1]
            if np.abs(gm - g).max() > 0:
                out[mut] = (gm, [n for n in every if n.startswith(('MDPA.query', 'MDPA.key'))])
    if case.prev is not None:                                        # two calls: what the call before left in the slab rows
        chain, prev = [], {}                                         # the slab rows keep what the latest call that wrote them left
        c0 = case
        while c0.prev is not None:
            c0 = S.BY_NAME[c0.prev]
            chain.append(c0)
        for earlier in reversed(chain):
            prev.update(_slots(earlier))
        mine = _slots(case)
        stale_first, stale_empty, stale_all = np.zeros_like(g), np.zeros_like(g), np.zeros_like(g)
        for idx, (c, rb, re_) in mine.items():
            if idx >= 2 * Lc['S'] or idx not in prev:                # the particles beyond the first two repeat them
                continue
            pc, pb, pe = prev[idx]
            left = G[pc, pb:pe].sum(axis=0)
            stale_all[c] += left
            (stale_first if re_ > rb else stale_empty)[c] += left
        if streamed:
            out['first-sequence-added-to-the-previous-call'] = (only(slab, g + stale_first), slab)
        if np.abs(stale_empty).max() > 0:
            out['empty-range-keeps-the-previous-call'] = (only(slab, g + stale_empty), slab)
        if case.family == 'wide':
            _, head, nq, tail = S.zero_fill(case)
            b, e = span[TABLE]
            for what, sl in (('head', slice(b, b + head)), ('tail', slice(e - tail, e))):
                if sl.stop > sl.start and np.abs(stale_all[:, sl]).max() > 0:
                    gm = g.copy()
                    gm[:, sl] += stale_all[:, sl]
                    out[f'table-{what}-not-zeroed'] = (gm, [TABLE])
    return out


MUTANT_KINDS = ('last-sequence-of-a-range-dropped', 'second-head-left-out', 'dq-dK-columns-dropped', 'score-tail-dropped', 'C-tail-dropped',
                'pad-positions-as-keys', 'duplicate-token-stored', 'second-sequence-stored', 'first-sequence-added-to-the-previous-call',
                'table-head-not-zeroed', 'table-tail-not-zeroed', 'empty-range-keeps-the-previous-call', 'dq_unscaled', 'ds_unmasked')
_SEEN = {}


@pytest.mark.parametrize('case', [c for c in S.CASES if c.N <= 40 and c.E <= 3 and c.prev is None][::7], ids=lambda c: c.name)
def test_the_second_restatement_is_the_first(case):
    """The torch model the forward-level mutants are built on gives tests/attn_ref.py's likelihood gradient, leaf by leaf at 1e-9."""
    P = S.problem(case)
    gl = P.lik(P.rows)
    gt = np.stack([_model(case, P, c, P.rows)[0] for c in range(2)])
    assert np.abs(gt - gl).max() <= 1e-9 * max(np.abs(gl).max(), 1e-300), case.name
    if case.K > 1:
        assert L.leaf_errors(gt, gl, P.leaves, {n: 'classifier.kernel' for n in S.zero_leaves(case, _names(P))}).max() < 1e-9


@pytest.mark.parametrize('case', S.CASES, ids=lambda c: c.name)
def test_a_wrong_schedule_misses_the_bound_tenfold(case):
    """Each mutant misses the GPU test's per-leaf bound by 10x or more on a leaf it touches, in both chains, and the float32
    evaluation of the case's own reference is inside the bound."""
    P = S.problem(case)
    names = _names(P)
    _, g, g32 = S.reference_of(case)
    bound = L.leaf_bounds(P.leaves, 2, g32, g, P.scale_of)
    L.assert_leaves(g32, g, P.leaves, bound, P.scale_of, tag=(case.name, 'float32 restatement'))
    for name, (g_mut, touched) in schedule_mutants(case).items():
        cols = [names.index(t) for t in touched]
        ratio = (L.leaf_errors(g_mut, g, P.leaves, P.scale_of) / bound)[:, cols].max(axis=1)
        _SEEN[name] = min(_SEEN.get(name, (np.inf, '')), (float(ratio.min()), case.name))
        assert ratio.min() >= 10.0, (case.name, name, ratio)
        with pytest.raises(AssertionError, match='leaf'):
            L.assert_leaves(g_mut, g, P.leaves, bound, P.scale_of, tag=name)


def test_every_kind_of_mutant_was_built(capsys):
    kinds = {}
    for c in S.CASES:
        if c.N > 40 and c.prev is None and not c.name.endswith('seq-full'):
            continue                                                # the row-range cases: their kinds are the small cases' too
        for name in schedule_mutants(c):
            kinds.setdefault(name, set()).add(c.family)
    assert set(kinds) == set(MUTANT_KINDS), set(MUTANT_KINDS) ^ set(kinds)
    for k in ('last-sequence-of-a-range-dropped', 'second-head-left-out', 'dq-dK-columns-dropped', 'score-tail-dropped', 'C-tail-dropped',
              'pad-positions-as-keys', 'dq_unscaled', 'ds_unmasked'):
        assert kinds[k] == set(S.FAMILIES), (k, kinds[k])
    assert kinds['duplicate-token-stored'] == {'attn', 'wide'} and kinds['empty-range-keeps-the-previous-call'] == {'attn', 'pre'}
    assert kinds['second-sequence-stored'] == kinds['first-sequence-added-to-the-previous-call'] == set(S.STREAMED)
    assert kinds['table-head-not-zeroed'] == kinds['table-tail-not-zeroed'] == {'wide'}
    if _SEEN:
        with capsys.disabled():
            print('\nATTNSCHED least miss of the bound per mutant: ' + ', '.join(f'{k} {v:.0f}x ({n})' for k, (v, n) in sorted(_SEEN.items())))

"""What one mile_step / mile_tune call launches on the update side, restated, the cases that put a launch into every cell of that
schedule, and the fp64 reference of one call (no torch, no GPU; tests/test_update_schedule_host.py proves the table on the CPU,
tests/test_gpu_update_schedule.py runs it).

The path (mile_amd/csrc/mile_hip.hip): mile_step and mile_tune build each launch's UpdParams with
upd_start / upd_mid / upd_record / chain_start and hand it to launch_update behind a gradient, or to the
gradient launch itself where fuse_ok lets k_grad_w64 run it as its epilogue.  launch_update picks k_update_fast
(launch_update_al: NK, nt, the compile-time kind of upd_kind, MAXT), k_update_big (launch_update_big),
k_update_seg + k_update_seg_scalars or the two-pass k_update<false>; row_align picks the vector width AL.  All of them
but the two-pass and the segment kernels run upd_fast_body (mile_update.h:560-904).  The epilogue form of that body is compiled
only under -DMILE_W64_EPILOGUE, which the build does not pass: its cells are listed as unreachable and its schedule is restated
for a library that has it (launches(case, epilogue=True)).  k_update<true> needs (d + 3) / 4 <= 4096
with d >> 2 == 0, i.e. d < 4; no FCN is that small (a regression net has at least F + 1 + 4 >= 6 parameters), so it is
unreachable from the FCN family and left out.

CELLS are projections of a launch, not the Cartesian product of its properties.  The pruning rule: a property is crossed with
another one only where one piece of code reads both.  The tail code (threads 0..ntail-1, scalar accesses) reads AL's quads only
through `to`, but shares the kind's folded flags, the noise source, SDC, out_sample and the g store with them, so (AL, ntail) is
crossed with each of those alone.  The scalar chain reads (kind, prior, refresh) and nothing of the geometry.  MAXT is a register
budget: crossed with the two forms that have it (TUNE, run-time) and AL (the width of the loads in flight).  The prefill
workgroups run upd_noise_body: (on / off) x (AL, ntail).  k_update_big draws its noise twice: (AL, ntail) x refresh.  The slab
sum is unrolled by four over S: S in {1, 2..4, >= 5}, read back from the launch info on the GPU.
"""
from __future__ import annotations

from collections import namedtuple
from functools import lru_cache

import numpy as np

# ---- constants of the code (tests/test_update_schedule_host.py parses them out of the sources) -----------------------------------
UPD_NT = 1024
UPD_QMAX = 4
UPD_QMAX_BIG = 9
UPD_SEG = 8192
SPLIT_768 = 768                 # launch_update_al: nt <= 768 takes the MAXT = 768 instantiation (TUNE kind, run-time form)
EPI_NT = 256                    # k_grad_w64's workgroup
EPILOGUE_ON = False             # MILE_W64_EPILOGUE_ON: the build does not define MILE_W64_EPILOGUE (mile_grad_w64.h:57-66)
FLAGS = dict(FROM_SLABS=1 << 0, START=1 << 1, B1=1 << 2, OA=1 << 3, RECORD=1 << 4, OB=1 << 5, B2=1 << 6, A=1 << 7, TUNE=1 << 8,
             NO_G=1 << 9)
_F = FLAGS
KIND_MID = _F['FROM_SLABS'] | _F['B1'] | _F['A'] | _F['NO_G']
KIND_REC = _F['FROM_SLABS'] | _F['B1'] | _F['OA'] | _F['RECORD'] | _F['OB'] | _F['B2'] | _F['A'] | _F['NO_G']
KIND_TUNE = _F['FROM_SLABS'] | _F['B1'] | _F['OA'] | _F['RECORD'] | _F['TUNE'] | _F['OB'] | _F['B2'] | _F['A']
STEP_START = _F['B2'] | _F['A']
STEP_RECORD = _F['FROM_SLABS'] | _F['B1'] | _F['OA'] | _F['RECORD']
KIND_NAMES = {KIND_MID: 'MID', KIND_REC: 'REC', KIND_TUNE: 'TUNE', -1: 'run-time'}
B1 = 0.1931833275037836
B2 = 1.0 - 2.0 * B1
N_CU = 256                      # MI355X; only generic_S reads it, and the GPU test checks S against the launch info
W64X3 = 'mfma_w64_bf16x3'

Case = namedtuple('Case', 'name F hidden N E mode n_steps refresh prior noise sdc kernel env off mask')


def _c(name, d, mode='step', n_steps=3, refresh='O-step-O', prior='Normal', noise='philox', sdc=False, E=2, N=16, env=(), off=0,
       mask=0, net=None, kernel='generic'):
    F, hidden = net if net else NETS[d]
    return Case(name, F, tuple(hidden), N, E, mode, n_steps, refresh, prior, noise, sdc, kernel, tuple(env), off, mask)


# d -> (F, hidden) of a regression FCN with that many parameters (bias + kernel per layer)
NETS = {
    6: (1, (1, 2)), 7: (2, (1, 2)), 256: (1, (1, 63, 2)), 257: (12, (17, 2)), 258: (5, (32, 2)), 3072: (7, (307, 2)),
    3073: (34, (83, 2)), 4095: (4, (49, 74, 2)), 4096: (43, (89, 2)), 4098: (29, (128, 2)), 4099: (14, (241, 2)),
    4100: (1, (16, 214, 2)), 8191: (1, (52, 147, 2)), 8193: (2, (38, 197, 2)), 8196: (31, (241, 2)), 12288: (3, (83, 139, 2)),
    12291: (2, (83, 140, 2)), 12292: (1, (55, 210, 2)), 16384: (1, (65, 239, 2)), 16386: (61, (256, 2)), 16387: (4, (77, 200, 2)),
    16388: (4, (74, 208, 2)), 16389: (1, (94, 167, 2)), 16390: (3, (79, 196, 2)), 20480: (4, (96, 202, 2)),
    20483: (3, (96, 203, 2)), 24577: (6, (140, 165, 2)), 28674: (3, (139, 198, 2)), 32771: (3, (144, 219, 2)),
    36864: (3, (176, 202, 2)), 36867: (2, (176, 203, 2)), 36868: (7, (167, 209, 2)), 36869: (1, (150, 239, 2)),
    40960: (1, (193, 207, 2)), 40961: (8, (159, 244, 2)), 40962: (7, (185, 210, 2)), 40963: (2, (167, 238, 2)),
}


def n_params(F, hidden):
    d, fin = 0, F
    for w in hidden:
        d += w + fin * w
        fin = w
    return d


def dim(case):
    return n_params(case.F, case.hidden)


# ---- the schedule ------------------------------------------------------------------------------------------------------------------

def ptr_align(off):
    """Alignment in floats of a pointer `off` floats behind a 16-byte aligned address (ptr_align in mile_hip.hip)."""
    return 4 if off % 4 == 0 else (2 if off % 2 == 0 else 1)


def row_align(d, ptrs):
    """(AL, why) of row_align: the width d allows, lowered by any non-null row pointer; ptrs: name -> offset."""
    al, why = (4, 'd % 4 == 0') if d % 4 == 0 else ((2, 'd % 2 == 0') if d % 2 == 0 else (1, 'd odd'))
    for off in ptrs.values():
        if ptr_align(off) < al:
            al, why = ptr_align(off), 'pointer'
    return al, why


def upd_fast_d(d):
    return 1 <= (d >> 2) <= UPD_NT * UPD_QMAX                                              # mile_update.h:994


def upd_kind(u):
    if u['prior'] != 'Normal' or u['sdc']:                                                 # mile_update.h:985-991
        return -1
    if u['flags'] == KIND_MID:
        return KIND_MID
    if u['flags'] == KIND_REC:
        return KIND_REC
    if u['flags'] == KIND_TUNE and 'u_rec' in u['ptrs']:
        return KIND_TUNE
    return -1


def threads(nqf, nk):
    return min(UPD_NT, ((nqf + nk - 1) // nk + 63) // 64 * 64)                              # 876, 911


def fuse_nk(nh):
    return ((8 * 64 + 64 + (nh - 1) * 4160 + 130) // 4 + 255) // 256                        # w64_fuse_nk<NH, 1>


def fuse_ok(case, u, epilogue=None):
    """fuse_ok on the probe `u`; `epilogue`: MILE_W64_EPILOGUE_ON, the build's unless given."""
    if not (EPILOGUE_ON if epilogue is None else epilogue):
        return False
    if case.kernel != W64X3 or u['sdc'] or 'u_rec' in u['ptrs']:
        return False
    nh = len(case.hidden) - 1
    if (case.F + 7) // 8 != 1:
        return False
    return (u['d'] >> 2) <= EPI_NT * fuse_nk(nh) and row_align(u['d'], u['ptrs'])[0] >= 2


def generic_S(N, E, n_cu=N_CU):
    return min(max(1, 2 * n_cu // max(E, 1)), max(1, N // 64), 64)                          # 228-232


def _reasons(u, kernel):
    """Why a launch runs the run-time-flag form, in the order the issue lists them."""
    f, out = u['flags'], []
    if f & _F['START']:
        out.append('start launch')
    if f & _F['RECORD'] and not f & (_F['A'] | _F['TUNE']):
        out.append('last record')
    if f & _F['RECORD'] and f & _F['A'] and not f & _F['OB']:
        out.append('step-O')
    if u['sdc']:
        out.append('SDC')
    if u['prior'] != 'Normal':
        out.append('Laplace')
    if f & _F['TUNE'] and 'u_rec' not in u['ptrs']:
        out.append('unmerged tuner')
    if kernel == 'big':
        out.append('big: no compile-time kinds')
    if kernel in ('seg', 'two-pass'):
        out.append(kernel + ': flags read at run time')
    return tuple(out)


def classify(case, u, fused):
    """The launch dict of UpdParams `u`: launch_update or the epilogue of the gradient launch."""
    d, E = u['d'], case.E
    nqf, ntail = d >> 2, d & 3
    env = set(case.env)
    al, why = row_align(d, u['ptrs'])
    ln = dict(d=d, ntail=ntail, nqf=nqf, flags=u['flags'], bits=tuple(k for k, v in FLAGS.items() if u['flags'] & v),
              prior=u['prior'], sdc=u['sdc'], AL=al, why=why, nwg=E, prefills=(), tuner=None, nseg=0, last_seg=0)
    if fused:
        ln.update(kernel='epilogue', NK=fuse_nk(len(case.hidden) - 1), nt=EPI_NT, MAXT=EPI_NT, AL=2, why='epilogue',
                  kind=upd_kind(u))
    elif upd_fast_d(d):                                                                     # 953-954
        nk = (nqf + UPD_NT - 1) // UPD_NT
        nt = threads(nqf, nk)
        kind = -1 if u['sdc'] else upd_kind(u)
        maxt = (SPLIT_768 if nt <= SPLIT_768 else UPD_NT) if kind in (KIND_TUNE, -1) else UPD_NT
        ln.update(kernel='fast', NK=nk, nt=nt, MAXT=maxt, kind=kind)
        if kind == KIND_MID and ('nz_A' in u['ptrs'] or 'nz_B' in u['ptrs']):               # 878
            ln.update(nwg=2 * E, prefills=tuple(k for k in ('nz_A', 'nz_B') if k in u['ptrs']))
    else:
        nk = (nqf + UPD_NT - 1) // UPD_NT
        big = (nqf >= 1 and UPD_QMAX < nk <= UPD_QMAX_BIG and not u['flags'] & _F['TUNE'] and u['zA'] != 'explicit'
               and u['zB'] != 'explicit' and 'MILE_NO_UPD_BIG' not in env)                  # 928
        if big:
            ln.update(kernel='big', NK=nk, nt=threads(nqf, nk), MAXT=UPD_NT, kind=-1)
        elif 'MILE_NO_UPD_SEG' not in env:                                                  # 943 (upart is always allocated)
            nseg = (d + UPD_SEG - 1) // UPD_SEG
            ln.update(kernel='seg', NK=0, nt=UPD_NT, MAXT=UPD_NT, kind=-1, nseg=nseg, last_seg=d - UPD_SEG * (nseg - 1))
        else:
            ln.update(kernel='two-pass', NK=0, nt=UPD_NT, MAXT=UPD_NT, kind=-1)
    ln['masked'] = ln['NK'] * ln['nt'] > nqf if ln['NK'] else False
    ln['kind_name'] = KIND_NAMES[ln['kind']]
    ln['reasons'] = _reasons(u, ln['kernel']) if ln['kind'] == -1 else ()

    def source(z, used):
        if not used:
            return None
        if z in ('explicit', 'prefilled'):
            return z
        return 'philox twice' if ln['kernel'] == 'big' else 'philox in place'
    ln['noiseA'] = source(u['zA'], u['flags'] & _F['OA'])
    ln['noiseB'] = source(u['zB'], u['flags'] & _F['OB'])
    ln['stores_g'] = bool(u['flags'] & _F['FROM_SLABS'] and not u['flags'] & _F['NO_G'])
    ln['out_sample'] = 'out_sample' in u['ptrs']
    if u['flags'] & _F['TUNE']:
        ln['tuner'] = dict(mask=u['t_mask'], merged='u_rec' in u['ptrs'], restart=bool(u.get('force_restart')))
    ln['stepB'], ln['stepA'] = u.get('stepB'), u.get('stepA')
    return ln


def _base(case, d, state_off):
    ptrs = {'x': state_off, 'u': state_off, 'g': state_off, 'slabs': 0}
    if case.sdc:
        ptrs['sdc'] = state_off                             # an offset case passes views of the preconditioner and the noise too
    return dict(d=d, prior=case.prior, sdc=case.sdc, ptrs=ptrs, flags=0, zA=None, zB=None)


def _copy(u):
    return dict(u, ptrs=dict(u['ptrs']))


def _chain_start(u, case, i):                                                               # 1806-1810
    u['flags'] |= STEP_START | (_F['OB'] if case.refresh == 'O-step-O' else 0)
    u['zB'] = 'explicit' if case.noise == 'explicit' else 'philox'
    if case.noise == 'explicit':
        u['ptrs']['zB'] = case.off
    u['stepB'] = i


def _upd_start(base, case, i):
    u = _copy(base)
    u['flags'] = _F['START']
    _chain_start(u, case, i)
    return u


def _upd_mid(base):
    u = _copy(base)
    u['flags'] = KIND_MID
    return u


def _upd_record(base, case, i):
    u = _copy(base)
    u['flags'] = STEP_RECORD
    u['zA'] = 'explicit' if case.noise == 'explicit' else 'philox'
    if case.noise == 'explicit':
        u['ptrs']['zA'] = case.off
    u['stepA'] = i
    return u


def launches(case, epilogue=None):
    """Every update launch of the call, in order (mile_step, mile_tune).  The pointer offsets: the caller's
    state `case.off` floats behind a 16-byte boundary, everything the library or the engine allocates on one.  `epilogue`: what
    the schedule would be in a library built with -DMILE_W64_EPILOGUE (the default build: EPILOGUE_ON)."""
    d, n, env = dim(case), case.n_steps, set(case.env)
    base = _base(case, d, case.off)
    out = []
    if case.mode == 'step':
        probe = _copy(base)
        if case.noise == 'explicit':
            probe['ptrs'].update(zA=case.off, zB=case.off)
        probe['ptrs']['out_sample'] = 0
        fused = fuse_ok(case, probe, epilogue)                                              # 3004-3006
        prefill = not fused and case.noise == 'philox' and upd_fast_d(d) and 'MILE_DEBUG=128' not in env   # 3010
        for i in range(n):
            if i == 0:
                out.append(classify(case, _upd_start(base, case, i), False))                # 3020: never fused
            ur = _upd_record(base, case, i)
            if i + 1 < n:
                _chain_start(ur, case, i + 1)
                ur['flags'] |= _F['NO_G']
            ur['ptrs']['out_sample'] = 0                                                    # n_thinning = 1
            u = _upd_mid(base)
            if prefill and upd_fast_d(d) and not u['sdc'] and upd_kind(u) == KIND_MID:      # 3031, update_prefills
                u['ptrs']['nz_A'] = 0
                ur['zA'] = 'prefilled'
                ur['ptrs']['zA'] = 0
                if ur['flags'] & _F['OB']:
                    u['ptrs']['nz_B'] = 0
                    ur['zB'] = 'prefilled'
                    ur['ptrs']['zB'] = 0
            out.append(classify(case, u, fused))
            out.append(classify(case, ur, fused))
        return out
    # mile_tune: A is the caller's state, B the library's
    A, B = case.off, 0
    if (d >> 2) > UPD_NT * UPD_QMAX or 'MILE_TUNE_POST' in env:                              # 3064-3090
        for i in range(n):
            out.append(classify(case, _upd_start(base, case, i), False))
            out.append(classify(case, _upd_mid(base), False))
            out.append(classify(case, _upd_record(base, case, i), False))
            out.append(dict(kernel='k_tune_post', d=d))
        return out
    no_merge, restart = 'MILE_TUNE_NO_MERGE' in env, 'MILE_TUNE_FORCE_RESTART' in env
    for i in range(n):
        cur, nxt = (B, A) if i & 1 else (A, B)

        def at(u, off):
            u['ptrs'].update(x=off, u=off, g=off)
        if i == 0 or no_merge:                                                              # 3104-3109
            u = _upd_start(base, case, i)
            at(u, nxt)
            u['ptrs'].update(x_in=cur, u_in=cur, g_in=cur)
            out.append(classify(case, u, False))
        u = _upd_mid(base)
        at(u, nxt)
        out.append(classify(case, u, False))
        ur = _upd_record(base, case, i)
        at(ur, nxt)
        ur['flags'] |= _F['TUNE']
        ur['t_mask'] = 1.0 if i < case.mask else 0.0                                        # schedule_step0 = 0
        ur['ptrs']['t_avg'] = 0
        if i + 1 < n and not no_merge:                                                      # 3119-3125
            _chain_start(ur, case, i + 1)
            ur['ptrs'].update(x_in=nxt, u_in=nxt, u_rec=nxt, x=cur, u=cur)
            ur['force_restart'] = restart
        out.append(classify(case, ur, False))
    return out


# ---- cells ---------------------------------------------------------------------------------------------------------------------------

TAILS = ((4, 0), (2, 2), (1, 1), (1, 3))
KINDS = ('MID', 'REC', 'TUNE', 'run-time')
SOURCES = ('explicit', 'philox in place', 'prefilled', 'philox twice')
REFRESH = ('O-step-O', 'step-O')


def s_class(S):
    return '1' if S == 1 else ('2..4' if S <= 4 else '>= 5')


def _enumerate_cells():
    cells = [('kernel', 'fast', nk) for nk in range(1, UPD_QMAX + 1)] + [('kernel', 'big', nk) for nk in range(UPD_QMAX + 1, UPD_QMAX_BIG + 1)]
    cells += [('kernel', 'epilogue', fuse_nk(2)), ('kernel', 'epilogue', fuse_nk(3)), ('kernel', 'two-pass', 0)]
    cells += [('seg', 5, 'ragged'), ('seg', 5, 8192), ('seg', 6, 1), ('seg', 6, 2), ('seg', 6, 3), ('seg', 3, 'ragged')]
    cells += [('lanes', 'nt 64, nqf 1')] + [('lanes', c, m) for c in ('nt <= 768', 'nt > 768') for m in (False, True)]
    cells += [('tail', al, nt, k) for al, nt in TAILS for k in KINDS]
    cells += [('tail-noise', al, nt, s) for al, nt in TAILS for s in SOURCES]
    cells += [('tail-sdc', al, nt) for al, nt in TAILS] + [('tail-sample', al, nt) for al, nt in TAILS]
    cells += [('tail-g', al, nt) for al, nt in TAILS]
    cells += [('kind', 'MID', 'Normal', r) for r in REFRESH] + [('kind', 'REC', 'Normal', 'O-step-O'), ('kind', 'TUNE', 'Normal', 'O-step-O')]
    cells += [('kind', why, 'Normal', r) for why in ('start launch', 'last record', 'SDC', 'unmerged tuner') for r in REFRESH]
    cells += [('kind', 'step-O', 'Normal', 'step-O')] + [('kind', 'Laplace', 'Laplace', r) for r in REFRESH]
    cells += [('kind', 'REC', 'Normal', 'step-O'), ('kind', 'TUNE', 'Normal', 'step-O')]
    cells += [('kind', k, 'Laplace', r) for k in ('MID', 'REC', 'TUNE') for r in REFRESH]
    cells += [('maxt', m, k, al) for m in (SPLIT_768, UPD_NT) for k in ('TUNE', 'run-time') for al in (4, 2, 1)]
    cells += [('prefill', on, al, nt) for on in (True, False) for al, nt in TAILS]
    cells += [('big-noise', al, nt, r) for al, nt in TAILS for r in REFRESH]
    cells += [('epilogue', nh, k, s) for nh in (2, 3) for k in ('MID', 'REC', 'run-time') for s in ('explicit', 'philox')]
    cells += [('al-by-pointer', al, k) for al in (2, 1) for k in ('MID', 'REC', 'big')]
    cells += [('slab-splits', c) for c in ('1', '2..4', '>= 5')]
    cells += [('hook', h) for h in ('MILE_NO_UPD_BIG', 'MILE_NO_UPD_SEG', 'MILE_DEBUG=128')]
    cells += [('one step', k) for k in ('fast', 'big', 'seg', 'epilogue')]
    # the tuner
    cells += [('tune', m, k, al, nt) for m in (SPLIT_768, UPD_NT) for k in ('TUNE', 'run-time') for al, nt in TAILS]
    cells += [('tune-nk', nk) for nk in range(1, UPD_QMAX + 1)] + [('tune', 'last merged d'), ('tune', 'k_tune_post')]
    cells += [('tune-hook', h, w) for h in ('MILE_TUNE_FORCE_RESTART', 'MILE_TUNE_NO_MERGE') for w in ('tail', 'MAXT 1024')]
    cells += [('tune-mask', mk, al, nt) for mk in (0, 2) for al, nt in TAILS]
    assert len(cells) == len(set(cells))
    return cells


CELLS = _enumerate_cells()

# cell -> the line that makes it unreachable
_NOT_REC = 'mile_hip.hip, chain_start: it adds UPD_OB only under O-step-O, so the chained word is not the kind\'s (static_asserts on UPD_KIND_REC / UPD_KIND_TUNE)'
_NOT_LAPLACE = 'mile_update.h:986: upd_kind returns -1 unless the prior is Normal'
_NO_EPILOGUE = ('mile_grad_w64.h:62-66 with mile_amd/_build.py: the library is built without -DMILE_W64_EPILOGUE, so MILE_W64_EPILOGUE_ON '
                'is 0 and fuse_ok (mile_hip.hip) refuses every launch; the body is not in the library')
UNREACHABLE = {('kind', 'REC', 'Normal', 'step-O'): _NOT_REC, ('kind', 'TUNE', 'Normal', 'step-O'): _NOT_REC}
UNREACHABLE.update({('kind', k, 'Laplace', r): _NOT_LAPLACE for k in ('MID', 'REC', 'TUNE') for r in REFRESH})
UNREACHABLE.update({c: _NO_EPILOGUE for c in CELLS if c[0] == 'epilogue' or c[:2] in (('kernel', 'epilogue'), ('one step', 'epilogue'))})


def cells_of(case):
    out = set()
    ls = [ln for ln in launches(case) if ln['kernel'] != 'k_tune_post']
    d = dim(case)
    tune = case.mode == 'tune'
    for ln in ls:
        k, al, nt, kind = ln['kernel'], ln['AL'], ln['ntail'], ln['kind_name']
        body = k in ('fast', 'big', 'epilogue')
        if k == 'seg':
            ls_ = ln['last_seg']
            out.add(('seg', ln['nseg'], ls_ if ls_ in (1, 2, 3, UPD_SEG) else 'ragged'))
        else:
            out.add(('kernel', k, ln['NK']))
        if body and not tune:
            if ln['nt'] == 64 and ln['nqf'] == 1:
                out.add(('lanes', 'nt 64, nqf 1'))
            elif k != 'epilogue':
                out.add(('lanes', 'nt <= 768' if ln['nt'] <= SPLIT_768 else 'nt > 768', ln['masked']))
        if k == 'fast' and not tune and ln['why'] != 'pointer':
            out.add(('tail', al, nt, kind))
            for s in (ln['noiseA'], ln['noiseB']):
                if s:
                    out.add(('tail-noise', al, nt, s))
            if ln['sdc']:
                out.add(('tail-sdc', al, nt))
            if ln['out_sample']:
                out.add(('tail-sample', al, nt))
            if ln['stores_g']:
                out.add(('tail-g', al, nt))
            if kind == 'MID' and case.noise == 'philox':
                out.add(('prefill', bool(ln['prefills']), al, nt))
            if kind == 'run-time':
                out.add(('maxt', ln['MAXT'], 'run-time', al))
        if k == 'fast' and tune and ln['tuner']:
            out.add(('tail', al, nt, kind))
            if ln['tuner']['merged']:
                out.add(('maxt', ln['MAXT'], kind, al))
                out.add(('tune', ln['MAXT'], kind, al, nt))
                out.add(('tune-nk', ln['NK']))
                if d == 4 * UPD_NT * UPD_QMAX + 3:
                    out.add(('tune', 'last merged d'))
            out.add(('tune-mask', case.mask, al, nt))
        if k == 'big' and ln['why'] != 'pointer':
            for s in (ln['noiseA'], ln['noiseB']):
                if s:
                    out.add(('tail-noise', al, nt, s))
                    out.add(('big-noise', al, nt, case.refresh))
        if k == 'epilogue':
            src = 'explicit' if case.noise == 'explicit' else 'philox'
            out.add(('epilogue', len(case.hidden) - 1, kind, src))
        if ln['why'] == 'pointer' and d % 4 == 0:
            if k == 'big':
                out.add(('al-by-pointer', al, 'big'))
            elif kind in ('MID', 'REC'):
                out.add(('al-by-pointer', al, kind))
        if kind != 'run-time':
            out.add(('kind', kind, case.prior, case.refresh))
        elif k == 'fast':                                        # the prior and the preconditioner decide before the flag word does
            why = ln['reasons']
            why = ('Laplace',) if 'Laplace' in why else (('SDC',) if 'SDC' in why else why)
            out |= {('kind', r, case.prior, case.refresh) for r in why}
    if tune and any(ln['kernel'] == 'k_tune_post' for ln in launches(case)):
        out.add(('tune', 'k_tune_post'))
    for h in ('MILE_NO_UPD_BIG', 'MILE_NO_UPD_SEG', 'MILE_DEBUG=128'):
        if h in case.env:
            out.add(('hook', h))
    for h in ('MILE_TUNE_FORCE_RESTART', 'MILE_TUNE_NO_MERGE'):
        if h in case.env:
            out.add(('tune-hook', h, 'tail' if d & 3 else 'MAXT 1024'))
            if d & 3 and any(ln.get('MAXT') == UPD_NT for ln in ls if ln.get('tuner')):
                out.add(('tune-hook', h, 'MAXT 1024'))
    if case.n_steps == 1 and case.mode == 'step':
        out.add(('one step', ls[-1]['kernel']))
    if case.kernel == 'generic':
        out.add(('slab-splits', s_class(generic_S(case.N, case.E))))
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
X, SO, LAP = 'explicit', 'step-O', 'Laplace'
CASES = [
    # k_update_fast, Philox: the MID and REC kinds with the prefill, every NK, both sides of every boundary
    _c('d6', 6, E=3), _c('d256', 256), _c('d257', 257, E=5), _c('d3073', 3073), _c('d4095', 4095), _c('d4096', 4096, E=3),
    _c('d4098', 4098), _c('d4100', 4100), _c('d8193', 8193), _c('d8196', 8196), _c('d12291', 12291), _c('d12292', 12292),
    _c('d16384', 16384), _c('d16386', 16386, N=8), _c('d16387', 16387, E=3),
    # explicit noise
    _c('d7-x', 7, noise=X, E=4), _c('d257-x', 257, noise=X), _c('d258-x', 258, noise=X), _c('d3072-x', 3072, noise=X),
    _c('d4099-x', 4099, noise=X), _c('d8191-x', 8191, noise=X), _c('d12288-x', 12288, noise=X, N=48),
    # step-O: the chained record launch in the run-time form, hA = 1
    _c('d257-so', 257, refresh=SO), _c('d4098-so-x', 4098, refresh=SO, noise=X), _c('d16387-so', 16387, refresh=SO),
    _c('d4096-so', 4096, refresh=SO), _c('d4099-so', 4099, refresh=SO),
    # Laplace prior: every launch in the run-time form
    _c('d258-lap', 258, prior=LAP), _c('d3073-lap-x', 3073, prior=LAP, noise=X), _c('d4099-lap-so-x', 4099, prior=LAP, refresh=SO, noise=X),
    _c('d4096-lap-so', 4096, prior=LAP, refresh=SO),
    # the preconditioner
    _c('d256-sdc-x', 256, sdc=True, noise=X), _c('d257-sdc', 257, sdc=True), _c('d4098-sdc', 4098, sdc=True),
    _c('d8191-sdc-x', 8191, sdc=True, noise=X), _c('d3072-sdc-so', 3072, sdc=True, refresh=SO),
    # every launch draws its own noise
    _c('d256-np', 256, env=('MILE_DEBUG=128',)), _c('d257-np', 257, env=('MILE_DEBUG=128',)),
    _c('d258-np', 258, env=('MILE_DEBUG=128',)), _c('d4099-np', 4099, env=('MILE_DEBUG=128',)), _c('d258', 258),
    # k_update_big: Philox only
    _c('d16388', 16388), _c('d16389-so', 16389, refresh=SO), _c('d16390', 16390), _c('d20480-so', 20480, refresh=SO),
    _c('d20483', 20483), _c('d24577', 24577), _c('d28674-so', 28674, refresh=SO), _c('d32771-so', 32771, refresh=SO),
    _c('d36864', 36864, E=3), _c('d36867', 36867), _c('d20483-sdc', 20483, sdc=True), _c('d16389-lap', 16389, prior=LAP),
    # k_update_seg: beyond 36867, or explicit noise beyond 16387
    _c('d36868', 36868), _c('d36869-x', 36869, noise=X), _c('d40960', 40960), _c('d40961-x', 40961, noise=X), _c('d40962', 40962),
    _c('d40963-so-x', 40963, noise=X, refresh=SO), _c('d16388-x', 16388, noise=X),
    _c('d16389-nobig', 16389, env=('MILE_NO_UPD_BIG',)), _c('d36869-noseg-x', 36869, noise=X, env=('MILE_NO_UPD_SEG',)),
    # one-step calls: the start launch and the last record launch alone
    _c('d257-n1', 257, n_steps=1), _c('d16389-n1', 16389, n_steps=1), _c('d40961-n1-x', 40961, n_steps=1, noise=X),
    # the nets whose updates would run as the epilogue of k_grad_w64 (ReLU regression on 64-wide layers, F <= 8) in a library
    # built with it; in the library as built they run k_update_fast behind mfma_w64_bf16x3's slabs
    _c('w64-nh2-x', 0, net=(5, (64, 64, 2)), kernel=W64X3, noise=X, N=48), _c('w64-nh2', 0, net=(8, (64, 64, 2)), kernel=W64X3, N=48),
    _c('w64-nh3-x', 0, net=(3, (64, 64, 64, 2)), kernel=W64X3, noise=X, N=48, E=3),
    _c('w64-nh3', 0, net=(8, (64, 64, 64, 2)), kernel=W64X3, N=48), _c('w64-nh2-n1', 0, net=(5, (64, 64, 2)), kernel=W64X3, N=48, n_steps=1),
    # more than one slab row per particle
    _c('d257-s4-x', 257, noise=X, N=256), _c('d258-s5', 258, N=320),
    # rows that are not 16-byte aligned although d % 4 == 0 (compared with the aligned call bit for bit)
    _c('d4096-off2', 4096, E=3, off=2), _c('d4096-off1', 4096, E=3, off=1), _c('d16388-off2', 16388, off=2), _c('d16388-off1', 16388, off=1),
    _c('d256-sdc-x-off2', 256, sdc=True, noise=X, off=2), _c('d256-sdc-x-off1', 256, sdc=True, noise=X, off=1),   # + noise and sdc views
]
T = 'tune'
CASES += [
    # the warm-up record kind: (MAXT) x (TUNE, run-time) x (AL, ntail), both masks
    _c('t3072', 3072, T, 2), _c('t258-x', 258, T, 2, noise=X, mask=2), _c('t3073', 3073, T, 2, mask=2), _c('t7-x', 7, T, 2, noise=X, E=3),
    _c('t4096-x', 4096, T, 2, noise=X, mask=2), _c('t4098', 4098, T, 2), _c('t8193', 8193, T, 2), _c('t4099', 4099, T, 2, mask=2),
    _c('t3072-sdc', 3072, T, 2, sdc=True, mask=2), _c('t258-lap', 258, T, 2, prior=LAP), _c('t3073-sdc-x', 3073, T, 2, sdc=True, noise=X),
    _c('t7-lap', 7, T, 2, prior=LAP, mask=2, E=3), _c('t4096-lap', 4096, T, 2, prior=LAP), _c('t4098-sdc-x', 4098, T, 2, sdc=True, noise=X, mask=2),
    _c('t8193-sdc', 8193, T, 2, sdc=True, mask=2), _c('t4099-lap-x', 4099, T, 2, prior=LAP, noise=X),
    _c('t258', 258, T, 2), _c('t3073-0', 3073, T, 2), _c('t7-2', 7, T, 2, mask=2, E=3), _c('t3072-2', 3072, T, 2, mask=2),
    _c('t4096', 4096, T, 2), _c('t4098-2', 4098, T, 2, mask=2), _c('t8193-2', 8193, T, 2, mask=2), _c('t4099-0', 4099, T, 2),
    _c('t12291', 12291, T, 2), _c('t16387-x', 16387, T, 2, noise=X), _c('t16388', 16388, T, 2),
    _c('t3073-restart', 3073, T, 2, env=('MILE_TUNE_FORCE_RESTART',)), _c('t4096-restart', 4096, T, 2, env=('MILE_TUNE_FORCE_RESTART',)),
    _c('t3073-nomerge', 3073, T, 2, env=('MILE_TUNE_NO_MERGE',)), _c('t4096-nomerge', 4096, T, 2, env=('MILE_TUNE_NO_MERGE',)),
    _c('t258-so', 258, T, 2, refresh=SO), _c('t4099-so-x', 4099, T, 2, refresh=SO, noise=X, mask=2),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
OFFSET_CASES = [c for c in CASES if c.off]
ORACLE_CASES = [c for c in CASES if not c.off]


def aligned_of(case):
    """The case an offset case is compared with."""
    return next(c for c in CASES if not c.off and c[1:] == case._replace(off=0)[1:])


# ---- problems --------------------------------------------------------------------------------------------------------------------
SEED, STEP_OFFSET = 0x5EED0123456789, 5
TUNE_KW = dict(desired_energy_var_start=0.5, desired_energy_var_end=0.1, trust_in_estimate=1.5, decay_rate=float(np.float32(99.0 / 101.0)))
TUNE_TOTAL = 67
KINK = 3e-7


def regime(d):
    """(prior_scale, eps factor) per size class, chosen so that delta = eps coef |g~| / (d - 1) of a B-step is near 1e-2: a wrong
    B-step then moves the displacement by ~1e-2 of itself against ~1e-5 of fp32 noise.  |g| is the prior's, |x| / scale^2 with
    |x| ~ 0.1 sqrt(d): delta ~ eps 0.019 / (scale^2 sqrt(d))."""
    if d <= 300:
        return 0.3, 10.0
    if d <= 5000:
        return 0.1, 10.0
    if d <= 17000:
        return 0.05, 10.0
    return 0.04, 10.0


def ospec_of(case):
    from oracle import mclmc_oracle as M
    act = 'relu' if case.kernel == W64X3 else 'tanh'
    return M.ModelSpec(case.F, case.hidden, activation=act, task='regr', prior=case.prior, prior_scale=regime(dim(case))[0])


def problem(case):
    return _problem(case._replace(name='', off=0, env=()))


@lru_cache(maxsize=None)
def _problem(case):
    """Everything both sides of a case are given, float32: X, y, theta0, eps, L, the preconditioner, the explicit noise (or the
    Philox seed, particle ids and step offset), the tuner's start.  Shared: treat as read-only."""
    from oracle import mclmc_oracle as M
    ospec, d, E = ospec_of(case), dim(case), case.E
    prob = M.synthetic_problem(ospec, case.N, E, seed=7)
    rng = np.random.default_rng(d * 31 + E)
    pb = dict(ospec=ospec, X=prob['X'], y=prob['y'], theta0=prob['theta0'], L=prob['L'],
              eps=(prob['eps'] * np.float32(regime(d)[1])).astype(np.float32), sdc=None, noise=None, z0=None,
              ids=(np.arange(E, dtype=np.int32) * 7919 + 13).astype(np.int32))
    if case.sdc:
        pb['sdc'] = (0.5 + rng.random((E, d))).astype(np.float32)
    if case.noise == 'explicit':
        pb['z0'] = rng.standard_normal((E, d)).astype(np.float32)
        pb['noise'] = rng.standard_normal((case.n_steps, 2, E, d)).astype(np.float32)
    if case.mode == 'tune':
        pb['eps_max'] = (pb['eps'] * np.float32(1.25)).astype(np.float32)
    for v in pb.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return pb


def host_start(case):
    """The fp32 start state of the host test: the fp64 oracle's mclmc_init rounded to float32 (the GPU test starts from the
    device's own eng.init instead)."""
    from oracle import mclmc_oracle as M
    pb = problem(case)
    f = lambda th: M.logpost_and_grad(pb['ospec'], th, pb['X'], pb['y'])
    z0 = pb['z0'] if pb['z0'] is not None else M.philox_normal(SEED, pb['ids'], 0, 2, dim(case))
    st = M.mclmc_init(f, pb['theta0'].astype(np.float64), np.asarray(z0, np.float64))
    return tuple(np.asarray(a, np.float32) for a in (st.position, st.momentum, st.logdensity, st.logdensity_grad))


# ---- the reference of one call, and what a wrong kernel would return ---------------------------------------------------------------
MUTANTS = ('tail-x-stale', 'tail-u-stale', 'tail-g-stale', 'tail-noise-quad-before', 'tail-noise-lane0', 'last-quad-skipped',
           'masked-lanes-counted', 'coef-swapped', 'hA-half-under-step-O', 'chained-O-old-counter', 'stages-swapped', 'divisor-d',
           'dK-not-restarted', 'lold-not-restarted', 'laplace-as-normal', 'sdc-not-in-A', 'big-pass2-other-stream',
           'seg-last-partials-dropped', 'sample-after-A', 'prefill-tail-missing',
           'tune-old-eps-next', 'tune-urec-post-O', 'tune-avg-old-weight', 'tune-avg-tail-stale')
DIVISOR_D_MAX = 300             # 'divisor-d' moves delta by 1 / d of itself: beyond this d no fp32 output can show it (see applies)


def applies(mut, case):
    """Whether the launches of `case` run the code the mutant breaks."""
    ls = [ln for ln in launches(case) if ln['kernel'] != 'k_tune_post']
    d = dim(case)
    ntail, nqf, philox, n = d & 3, d >> 2, case.noise == 'philox', case.n_steps
    body = [ln for ln in ls if ln['kernel'] in ('fast', 'big', 'epilogue')]
    tune, oso = case.mode == 'tune', case.refresh == 'O-step-O'
    merged = any(ln['tuner'] and ln['tuner']['merged'] for ln in ls)
    return {
        'tail-x-stale': ntail > 0, 'tail-u-stale': ntail > 0, 'tail-g-stale': ntail > 0 and not tune,
        'tail-noise-quad-before': philox and ntail > 0 and bool(body), 'tail-noise-lane0': philox and ntail >= 2 and bool(body),
        'last-quad-skipped': bool(body) and ntail == 0 and all(nqf % ln['nt'] == 0 for ln in body),
        'masked-lanes-counted': bool(body) and all(ln['masked'] for ln in body),
        'coef-swapped': True, 'hA-half-under-step-O': not oso, 'chained-O-old-counter': n >= 2 and oso and (not tune or merged),
        'stages-swapped': True,
        # the scalar chain's divisor: a relative change of 1 / d in delta.  At d = 16388 that is 6e-5 of a delta of 1e-2, i.e.
        # 6e-7 of the momentum's largest entry and (through u.e ~ 1 / sqrt(d)) 5e-7 of the kinetic scale: below what float32
        # resolves on any output.  So it is measured where 1 / d is large, on upd_fast_body alone.
        'divisor-d': d <= DIVISOR_D_MAX and bool(body),
        'dK-not-restarted': n >= 2 and not tune, 'lold-not-restarted': n >= 2 and not tune,
        'laplace-as-normal': case.prior == 'Laplace', 'sdc-not-in-A': case.sdc,
        'big-pass2-other-stream': any(ln['kernel'] == 'big' for ln in ls) and oso,
        'seg-last-partials-dropped': any(ln['kernel'] == 'seg' for ln in ls),
        'sample-after-A': n >= 2 and not tune,
        'prefill-tail-missing': ntail > 0 and any(ln['prefills'] for ln in ls),
        'tune-old-eps-next': tune and merged, 'tune-urec-post-O': tune and merged and 'MILE_TUNE_FORCE_RESTART' in case.env and oso,
        'tune-avg-old-weight': tune and case.mask == 0, 'tune-avg-tail-stale': tune and case.mask == 0 and ntail > 0,
    }[mut]


def _weights(case, mut, d):
    """(w, keep): the weight of each element in the dot products, and the elements a launch updates."""
    w, upd = np.ones(d), np.ones(d, bool)
    ls = [ln for ln in launches(case) if ln['kernel'] != 'k_tune_post']
    if mut == 'last-quad-skipped':
        q = (d >> 2) - 1
        w[4 * q:4 * q + 4] = 0.0
        upd[4 * q:4 * q + 4] = False
    if mut == 'masked-lanes-counted':
        ln = next(l for l in ls if l['masked'])
        w[:4] += ln['NK'] * ln['nt'] - (d >> 2)                                             # the clamped loads read quad 0
    if mut == 'seg-last-partials-dropped':
        w[UPD_SEG * ((d + UPD_SEG - 1) // UPD_SEG - 1):] = 0.0
    return w, upd


def simulate(case, start, dtype=np.float64, mut=None):
    """One mile_step / mile_tune call of `case` from the float32 state `start` = (x, u, logp, g), every array in `dtype`, in the
    oracle's arithmetic (tests/test_update_schedule_host.py holds the float64 form to oracle.mclmc_step / oracle.tuner_step).
    The kinetic change is the stable form Chain::B uses.  `mut` names one plausible kernel error (MUTANTS).  Returns a dict:
    samples [n, E, d] (x at every record point, as out_sample sees it), x, u, g, logp (final), info [n, E, 3], sK [n, E] (the
    kinetic scale of each step), grad_points [2n, E, d] (where the gradient was taken), and for the tuner eps, eps_max, time, x_average, W, avg."""
    from oracle import mclmc_oracle as M
    dt = np.dtype(dtype).type
    pb, d, E, n = problem(case), dim(case), case.E, case.n_steps
    ospec = pb['ospec']
    if mut == 'laplace-as-normal':
        ospec = M.ModelSpec(case.F, case.hidden, activation=ospec.activation, task='regr', prior='Normal', prior_scale=ospec.prior_scale)
    Xd, yd = pb['X'].astype(dt), pb['y'].astype(dt)
    f = lambda th: M.logpost_and_grad(ospec, th, Xd, yd)
    x, u, logp, g = (np.array(a, dtype=dt) for a in start)
    g_start = g.copy()
    L = pb['L'].astype(dt)
    sdc = pb['sdc'].astype(dt) if pb['sdc'] is not None else dt(1.0)
    nqf, ntail, tail = d >> 2, d & 3, slice(4 * (d >> 2), d)
    w, upd = _weights(case, mut, d)
    w = w.astype(dt)
    oso, tune = case.refresh == 'O-step-O', case.mode == 'tune'
    prefilled = any(ln['prefills'] for ln in launches(case) if ln['kernel'] != 'k_tune_post')

    def noise(i, stage, step=None, other=False):
        step = i if step is None else step
        if mut == 'stages-swapped' or other:
            stage = 1 - stage
        if pb['noise'] is not None:
            return pb['noise'][step, stage].astype(dt)
        z = M.philox_normal(SEED, pb['ids'], STEP_OFFSET + step, stage, d, dtype=dt).copy()
        if ntail and mut == 'tail-noise-quad-before':
            z[:, tail] = z[:, 4 * (nqf - 1):4 * (nqf - 1) + ntail]
        if ntail and mut == 'tail-noise-lane0':
            z[:, tail] = z[:, 4 * nqf:4 * nqf + 1]
        if ntail and mut == 'prefill-tail-missing' and prefilled and (stage == 1 or i > 0):
            z[:, tail] = 0
        return z

    def dot(a, b):
        return (w * a * b).sum(axis=-1, keepdims=True)

    def put(new, old, what):
        """What the launch leaves in memory: `new`, except where the mutant keeps the old value."""
        out = np.where(upd, new, old)
        if ntail and mut == f'tail-{what}-stale':
            out[:, tail] = old[:, tail]
        return out

    def Bstep(u, g, eps, coef):
        gs = g * sdc
        gn = np.sqrt(dot(gs, gs))
        e = gs / gn
        ue = dot(u, e)
        delta = eps[:, None] * dt(coef) * gn / dt(d if mut == 'divisor-d' else d - 1)
        zeta = np.exp(-delta)
        uu = e * (1 - zeta) * (1 + zeta + ue * (1 - zeta)) + 2 * zeta * u
        un = uu / np.sqrt(dot(uu, uu))
        dK = dt(d - 1) * (delta + np.log1p(dt(0.5) * (1 - ue) * np.expm1(-2 * delta)))
        return put(un.astype(dt), u, 'u'), dK[:, 0].astype(dt), gn[:, 0]

    def Ostep(u, z, h, z_apply=None):
        nu = np.sqrt(np.expm1(dt(2.0) * h / L) / dt(d)).astype(dt)[:, None]
        v = u + nu * z
        va = v if z_apply is None else u + nu * z_apply
        return put((va / np.sqrt(dot(v, v))).astype(dt), u, 'u')

    def Astep(x, u, eps):
        s = dt(1.0) if mut == 'sdc-not-in-A' else sdc
        return put((x + (eps[:, None] * dt(0.5)) * (u * s)).astype(dt), x, 'x')

    c1, c2, c3 = (B2, B1, B1) if mut == 'coef-swapped' else (B1, B2, B1)
    eps = pb['eps'].astype(dt)
    if tune:
        ad = M.AdaptiveState(np.zeros(E, dt), np.zeros(E, dt), pb['eps_max'].astype(dt), np.zeros(E, dt), np.zeros((E, 2, d), dt))
    samples, infos, sKs, eps_used, pts = [], [], [], [], []
    dk_carry, lold0 = np.zeros(E, dt), logp.copy()
    big2 = mut == 'big-pass2-other-stream'
    eps_first = eps                       # the step size of the step's O(z1), B(b1), A: the merged launch forms them
    for i in range(n):
        lold = logp
        if oso:
            zi = noise(i, 0, step=i - 1 if (mut == 'chained-O-old-counter' and i > 0) else None)
            u = Ostep(u, zi, dt(0.5) * eps_first, noise(i, 0, other=True) if big2 else None)
            if mut == 'tune-urec-post-O' and i > 0:
                u = Ostep(u, zi, dt(0.5) * eps_first)
        u, dK1, gn0 = Bstep(u, g, eps_first, c1)
        x = Astep(x, u, eps_first)
        if mut == 'sample-after-A' and i > 0:
            samples[-1] = x.copy()                                                          # written behind the chained A-step
        pts.append(x)
        g = f(x)[1].astype(dt)
        u, dK2, gn1 = Bstep(u, g, eps, c2)
        x = Astep(x, u, eps)
        pts.append(x)
        logp, g = f(x)
        logp, g = logp.astype(dt), g.astype(dt)
        u, dK3, gn2 = Bstep(u, g, eps, c3)
        hA = dt(0.5) if (oso or mut == 'hA-half-under-step-O') else dt(1.0)
        u = Ostep(u, noise(i, 1), hA * eps, noise(i, 1, other=True) if big2 else None)
        dK = dK1 + dK2 + dK3
        if mut == 'dK-not-restarted':
            dk_carry = dk_carry + dK
            dK = dk_carry
        dE = dK - (logp - (lold0 if mut == 'lold-not-restarted' else lold))
        infos.append(np.stack([logp, dK, dE], axis=1))
        sKs.append(eps_first * dt(B1) * gn0 + eps * (dt(B2) * gn1 + dt(B1) * gn2))
        samples.append(x.copy())
        eps_used.append(eps)
        if tune:
            var = M.desired_energy_var(i, TUNE_TOTAL, TUNE_KW['desired_energy_var_start'], TUNE_KW['desired_energy_var_end'])
            ad.step_size_max = np.nan_to_num(ad.step_size_max)
            eps_new, _, _ = M.predictor_update(dE.astype(dt), eps, ad, dim=d, var=dt(np.float32(var)),
                                               trust_in_estimate=TUNE_KW['trust_in_estimate'], decay=dt(TUNE_KW['decay_rate']))
            mask = 1.0 if i < case.mask else 0.0
            wgt = ((1 - mask) * (eps if mut == 'tune-avg-old-weight' else eps_new)).astype(dt)
            avg_old = ad.avg
            ad.W, ad.avg = M.streaming_average_update(np.stack([x, x * x], axis=1), (ad.W, ad.avg), weight=wgt,
                                                      zero_prevention=np.full(E, mask, dtype=dt))
            ad.avg = ad.avg.astype(dt)
            if mut == 'tune-avg-tail-stale' and ntail:
                ad.avg[:, :, tail] = avg_old[:, :, tail]
            eps_first = eps if mut == 'tune-old-eps-next' else eps_new
            eps = eps_new
    g_out = g.copy()
    if ntail and mut == 'tail-g-stale':
        g_out[:, tail] = g_start[:, tail]
    out = dict(samples=np.stack(samples), x=x, u=u, g=g_out, logp=logp, info=np.stack(infos), sK=np.stack(sKs), x0=np.array(start[0], dt),
               grad_points=np.stack(pts))
    if tune:
        out.update(eps=eps, eps_max=ad.step_size_max, time=ad.time, x_average=ad.x_average, W=ad.W, avg=ad.avg,
                   eps_used=np.stack(eps_used))
    return out


# ---- the comparison ------------------------------------------------------------------------------------------------------------------
QUANTITIES = ('displacement', 'momentum', 'unit norm', 'logdensity', 'kinetic change', 'energy change', 'gradient',
              'stream weight', 'stream average')
# One bound per quantity for the whole table.  tests/test_update_schedule_host.py recomputes r_q (the float32 evaluation's own
# error) and m_q (the least miss of a mutant that this quantity is the one to catch) and asserts 8 r_q <= B_q <= m_q / 10.
BOUNDS = {
    'displacement': 2e-4,       # of the particle's largest oracle displacement + 2 fp32 ulps of max |x|
    'momentum': 5e-5,           # of the particle's largest |u|
    'unit norm': 2e-6,          # | |u| - 1 |
    'logdensity': 2e-5,         # relative
    'kinetic change': 3e-5,     # of s_K = eps (b1 |g~0| + b2 |g~1| + b1 |g~2|)
    'energy change': 1.0,       # of BOUNDS['kinetic change'] s_K + 16 fp32 ulps of max |logp|
    'gradient': 2e-5,           # of its largest entry (the parity table's bound)
    'stream weight': 1e-5,      # of its largest entry
    'stream average': 1e-5,     # of its largest entry
}


def _f64(a):
    return np.asarray(a, np.float64)


def errors(got, ref, case):
    """{quantity: worst normalised error} of a result against the fp64 reference `ref` (both dicts of simulate's shape; the
    device's result is put into that shape by the GPU test)."""
    if case.mode == 'tune':                                  # mile_tune returns no samples: the displacement of the whole call
        xs_g, xs_r = np.stack([_f64(ref['x0']), _f64(got['x'])]), np.stack([_f64(ref['x0']), _f64(ref['x'])])
    else:
        xs_g = np.concatenate([_f64(ref['x0'])[None], _f64(got['samples'])])
        xs_r = np.concatenate([_f64(ref['x0'])[None], _f64(ref['samples'])])
    dg, dr = np.diff(xs_g, axis=0), np.diff(xs_r, axis=0)
    floor = 2.0 * np.spacing(np.abs(xs_r).max(axis=(0, 2)).astype(np.float32)).astype(np.float64)      # [E]
    out = {'displacement': float((np.abs(dg - dr).max(axis=2) / (np.abs(dr).max(axis=2) + floor)).max())}
    ur = _f64(ref['u'])
    out['momentum'] = float((np.abs(_f64(got['u']) - ur).max(axis=1) / np.abs(ur).max(axis=1)).max())
    out['unit norm'] = float(np.abs(np.linalg.norm(_f64(got['u']), axis=1) - 1.0).max())
    ig, ir = _f64(got['info']), _f64(ref['info'])
    lp = np.concatenate([np.abs(ig[..., 0] - ir[..., 0]) / np.abs(ir[..., 0]), (np.abs(_f64(got['logp']) - ref['logp']) / np.abs(ref['logp']))[None]])
    out['logdensity'] = float(lp.max())
    sK = _f64(ref['sK'])
    out['kinetic change'] = float((np.abs(ig[..., 1] - ir[..., 1]) / sK).max())
    ulp = float(np.spacing(np.float32(np.abs(ir[..., 0]).max())))
    out['energy change'] = float((np.abs(ig[..., 2] - ir[..., 2]) / (BOUNDS['kinetic change'] * sK + 16 * ulp)).max())
    gr = _f64(ref['g'])
    out['gradient'] = float((np.abs(_f64(got['g']) - gr).max(axis=1) / np.abs(gr).max(axis=1)).max())
    if case.mode == 'tune':
        out['stream weight'] = float(np.abs(_f64(got['W']) - ref['W']).max() / max(np.abs(ref['W']).max(), 1e-30))
        out['stream average'] = float(np.abs(_f64(got['avg']) - ref['avg']).max() / max(np.abs(ref['avg']).max(), 1e-30))
    return out


def worst_ratio(err):
    """(quantity, error / bound) of the quantity that misses its bound by most."""
    q = max(err, key=lambda k: err[k] / BOUNDS[k])
    return q, err[q] / BOUNDS[q]

"""The edges of a k_grad_w64 launch -- weight staging in front of the first row block, the cross-wave reduction and the slab
stores behind the last -- on the smallest shapes in which every path of both runs (-m gpu).

Forms: mfma_w64_bf16x3 and mfma_w64 with two and three hidden layers and F = 5 (one X quad per row) and 12 (two).  Cases, at
E = 3 particles (particle 2 repeats particle 0's parameters):

    N = 27    one workgroup, one ragged block: no main-loop round, the block shared by wave pair 0 while pair 1 only counts barriers
    N = 59    one workgroup, two blocks: no main-loop round, one shared block per wave pair (the pair tail alone)
    N = 283   two workgroups with 4 and 5 blocks: one main-loop round each, then nothing / one block shared by pair 0

so staging is followed by a tail block directly and by a main-loop round, the reduction adds waves that did and did not take
part in a tail, and S = 1 and S = 2 slabs per particle are written.

Checks.  (1) Log-density and every gradient leaf of particles 0 and 1 against the fp64 oracle with the per-leaf check and the
tolerances of tests/leafcheck.py, the whole gradient and the log-density at the 2e-5 of tests/test_gpu_w64_schedule.py.
(2) Particle 2 equals particle 0 bit for bit.  (3) Bit for bit against the commit before the staging was pipelined:
tests/golden/w64_edges_parent.json holds, for every form and case, the SHA-256 of the float32 log-densities and gradients that
build returned on an MI355X for these inputs (written by tests/golden/make_w64_edges_digests.py, which says how).  The library does not expose the slabs; the gradient is k_finalize's
sum_s slab[s] - grad log prior, an unchanged kernel, so equal slabs give equal digests, and a slab that moved by one ulp moves
the gradient unless the prior term's rounding hides it.  (The slabs themselves were compared in the lab harness on the
benchmark's shape, tools/r10/lab/w64_edges_lab.hip: profiles/r10/.)

The scalar-store path of the reduction (`w_off & 3 != 0`) is not reachable: the kernel only runs nets whose hidden layers are all
64 wide, whose layout (bias before kernel, layer after layer) puts every hidden kernel at a multiple of 64 floats, whatever F.
"""
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

from tests import leafcheck as L
from tests import w64_schedule as W

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

DEV = 'cuda:0'
E = 3
LP_TOL = 2e-5            # relative, tests/test_gpu_w64_schedule.py
WHOLE_TOL = 2e-5         # of the gradient's largest entry, the same
FORMS = [(F, (64,) * nh + (2,), k) for k in ('mfma_w64_bf16x3', 'mfma_w64') for nh in (2, 3) for F in (5, 12)]
CASES = {27: [1], 59: [2], 283: [4, 5]}          # N -> blocks per workgroup at E = 3
GOLDEN = Path(__file__).resolve().parent / 'golden' / 'w64_edges_parent.json'


def key_of(form, N):
    return f'{W.form_id(form)}-N{N}'


def digest(lp, g):
    """SHA-256 over the float32 bytes of the log-densities, then the gradients, of particles 0 and 1."""
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(lp, dtype=np.float32).tobytes())
    h.update(np.ascontiguousarray(g, dtype=np.float32).tobytes())
    return h.hexdigest()


def run(form, N):
    """One launch of `form` on N rows and E particles: (grid, logp [E], gradient [E, d]) as float32 arrays."""
    from mile_amd import ModelSpec
    from mile_amd.engine import Engine
    F, hs, kernel = form
    _, X, y, theta = W.problem(form, N, E, W.seed_of(form, N))
    eng = Engine(ModelSpec(in_features=F, hidden_structure=hs), torch.from_numpy(X), torch.from_numpy(y), device=DEV, grad_kernel=kernel)
    assert eng.grad_kernel == kernel
    info = eng.grad_launch_info(E)
    lp, g = eng.logpost_grad(torch.from_numpy(theta))
    torch.cuda.synchronize()
    return info, lp.cpu().numpy(), g.cpu().numpy()


@pytest.mark.parametrize('N', list(CASES), ids=[f'N{n}' for n in CASES])
@pytest.mark.parametrize('form', FORMS, ids=[W.form_id(f) for f in FORMS])
def test_launch_edges(form, N):
    fid, net = W.form_id(form), (form[0], form[1])
    info, lp, g = run(form, N)
    # the cell: the launch is the one the case was chosen for
    S = W.splits(N, E)
    assert info['kernel'] == 'k_grad_w64' and info['grid'] == (S, E), (fid, N, info)
    assert W.blocks(N, S) == CASES[N], (fid, N, W.blocks(N, S))
    # (1) the oracle
    lp_ref, g_ref, g32 = W.reference(net, N, W.seed_of(form, N))
    leaves = L.fcn_leaves(W.ospec_of(net))
    bound = L.leaf_bounds(leaves, 2, g32=g32, g_ref=g_ref, tol=L.LEAF_TOL, margin=L.F32_MARGIN)
    g2 = g[:2].astype(np.float64)
    e_lp = np.abs(lp[:2].astype(np.float64) - lp_ref).max() / np.abs(lp_ref).max()
    e_whole = np.abs(g2 - g_ref).max(axis=1) / np.abs(g_ref).max(axis=1)
    err = L.leaf_errors(g2, g_ref, leaves)
    print(f'\nW64EDGE {fid} N{N} grid {info["grid"]}: logp {e_lp:.2e}  whole {e_whole.max():.2e}  worst leaf {err.max():.2e} '
          f'(bound {bound.min():.2e}..{bound.max():.2e})')
    assert np.isfinite(lp).all() and np.isfinite(g).all(), (fid, N)
    assert e_lp < LP_TOL, (fid, N, e_lp)
    assert e_whole.max() < WHOLE_TOL, (fid, N, e_whole)
    L.assert_leaves(g2, g_ref, leaves, bound, tag=(fid, N))
    # (2) the replica
    assert np.array_equal(lp[2], lp[0]) and np.array_equal(g[2], g[0]), (fid, N)
    # (3) the commit before
    want = json.loads(GOLDEN.read_text())
    got = digest(lp[:2], g[:2])
    print(f'W64EDGE {fid} N{N}: digest {got[:16]}  parent {want[key_of(form, N)][:16]}')
    assert got == want[key_of(form, N)], (fid, N, 'log-density or gradient differs from the parent build bit-wise')

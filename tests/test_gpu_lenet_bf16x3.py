"""`lenet_bf16x3` (MILE_GRAD_LENET_BF16X3): LeNet's five convolution products on the bf16 matrix pipe from exact three-term
splits of both operands, six MFMA products per accumulator -- held to the bounds of the fp32 path (`lenet_f32` in
tests/test_gpu_lenet.py) against the plain fp64 oracle, not to the bf16 recipe (-m gpu).

Images per barrier pair (mile_hip.hip, lenet_ni_for with three term planes): ni = clamp(57344 // (3 * bytes per image), 1, 4)
    conv1 forward       bytes = ((H + 4)(W + 4) + 8) * 8
    conv2 fwd / dW      bytes = (hp * wp + 8) * 16 + h2 * w2 * 32        hp = H // 2, h2 = hp - 4
    conv2 dX            bytes = ((h2 + 8)(w2 + 8) + 8) * 32

ReLU cases: one Dense unit on the kink moves a leaf by ~1/N in an fp64-vs-fp32 comparison whatever the kernel, so every ReLU
case first asserts (in fp64) that each Dense pre-activation is farther than 5e-6 of its layer's largest from zero."""
import numpy as np
import pytest

from oracle import lenet_oracle as LN
from oracle import mclmc_oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

KERNEL = 'lenet_bf16x3'


def _ospec(C, H, W, K, act='relu', task='classification', prior='Normal'):
    return LN.LeNetSpec(C, H, W, K, activation=act, task=task, prior=prior, prior_scale=0.7 if prior == 'Laplace' else 1.0)


def _engine(ospec, X, y, kernel=KERNEL):
    from mile_amd import LeNetSpec
    from mile_amd.engine import Engine
    spec = LeNetSpec(ospec.channels, ospec.height, ospec.width, ospec.out_dim, activation=ospec.activation, task=ospec.task,
                     prior=ospec.prior, prior_loc=ospec.prior_loc, prior_scale=ospec.prior_scale)
    eng = Engine(spec, torch.from_numpy(X), torch.from_numpy(y), device='cuda:0', grad_kernel=kernel)
    assert eng.grad_kernel == kernel
    return eng


def _relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _assert_off_the_kink(ospec, th64, X):
    if ospec.activation != 'relu':
        return
    _, c = LN.forward(ospec, th64, X, keep=True)
    for k in ('zf1', 'zf2'):
        m = np.abs(c[k]).min() / np.abs(c[k]).max()
        assert m > 5e-6, (k, m)


def _check_grad(ospec, prob, sl=slice(None), eng=None, lp_tol=2e-5, g_tol=5e-5):
    """lp and every parameter leaf (relative to the leaf's largest entry) against the fp64 oracle on rows sl."""
    th64 = prob['theta0'].astype(np.float64)
    X, y = prob['X'][sl], prob['y'][sl]
    _assert_off_the_kink(ospec, th64, X)
    lp_ref, g_ref = LN.logpost_and_grad(ospec, th64, X, y)
    eng = eng or _engine(ospec, prob['X'], prob['y'])
    lp, g = eng.logpost_grad(torch.from_numpy(prob['theta0']))
    torch.cuda.synchronize()
    g = g.cpu().numpy()
    errs = {name: _relerr(g[:, off:off + int(np.prod(shape))], g_ref[:, off:off + int(np.prod(shape))]) for name, off, shape in ospec.leaves()}
    e_lp = _relerr(lp.cpu().numpy(), lp_ref)
    print(f'{ospec.channels}x{ospec.height}x{ospec.width}: lp {e_lp:.2e}, worst leaf {max(errs.values()):.2e}')
    assert e_lp < lp_tol, e_lp
    for name, e in errs.items():
        assert e < g_tol, (name, e)


CASES = [
    # C, H, W, out_dim, activation, task, prior, N, E, seed  (tests/test_gpu_lenet.py CASES + the two of its MFMA test)
    (1, 28, 28, 10, 'relu', 'classification', 'Normal', 37, 3, 203),   # MNIST-shaped; seed 3 has an fc1 unit 1.4e-6 from the kink
    (3, 32, 32, 10, 'relu', 'classification', 'Normal', 20, 4, 3),     # CIFAR-shaped (config 5): ni 1 / 2 / 1
    (2, 13, 17, 2, 'tanh', 'regr', 'Laplace', 9, 2, 3),                # odd sizes: pooling crops a row and a column
    (1, 12, 12, 3, 'sigmoid', 'classification', 'Normal', 1, 1, 3),    # smallest image, one row, one particle
    (4, 20, 24, 4, 'relu', 'classification', 'Normal', 19, 2, 3),      # four input channels: a full slot
    (3, 18, 22, 5, 'relu', 'classification', 'Normal', 7, 2, 3),       # conv2's input is 9 x 11: odd width in the pair forms
]


@pytest.mark.parametrize('C,H,W,K,act,task,prior,N,E,seed', CASES)
def test_gradient_matches_fp64_at_the_fp32_bounds(C, H, W, K, act, task, prior, N, E, seed):
    ospec = _ospec(C, H, W, K, act, task, prior)
    _check_grad(ospec, LN.synthetic_problem(ospec, N, E, seed=seed))


@pytest.mark.parametrize('C,H,W', [(1, 12, 13), (2, 15, 12), (3, 21, 19), (4, 14, 30), (1, 33, 12), (3, 12, 37), (2, 26, 26)])
def test_geometry_sweep(C, H, W):
    """The tile / pair / chunk boundaries of test_lenet_mfma_geometry_sweep, where ni now differs from the bf16 kernel's."""
    ospec = _ospec(C, H, W, 3)
    _check_grad(ospec, LN.synthetic_problem(ospec, 5, 2, seed=11))


@pytest.mark.parametrize('C,H,W', [
    (1, 36, 36),   # conv1 ni = 57344 // (3 * 12864) = 1; conv2 (18 x 18 -> 14 x 14) ni = 57344 // (3 * 11584) = 1; dX ni = 1
    (2, 22, 22),   # conv1 ni = 57344 // (3 * 5472) = 3; conv2 (11 x 11 -> 7 x 7) ni = min(4, 57344 // (3 * 3632)) = 4; dX ni = 2
    (1, 12, 12),   # every launch at the maximum, ni = 4 (conv1 3 * 2112 bytes, conv2 3 * 832, dX 3 * 3456)
])
def test_images_per_barrier_pair_boundaries(C, H, W):
    """ni = 1, 2, 3 and the maximum 4, with N = 5 images so that a last group is short of ni (MNIST and CIFAR above: 2 / 2 / 1, 1 / 2 / 1)."""
    ospec = _ospec(C, H, W, 3)
    _check_grad(ospec, LN.synthetic_problem(ospec, 5, 2, seed=11))


def test_image_chunks_accumulate(monkeypatch):
    monkeypatch.setenv('MILE_GEMM_ROWS', '4')
    ospec = _ospec(3, 16, 20, 5)
    _check_grad(ospec, LN.synthetic_problem(ospec, 11, 3, seed=5))


def test_row_windows():
    ospec = _ospec(3, 16, 16, 4)
    prob = LN.synthetic_problem(ospec, 41, 2, seed=19)
    eng = _engine(ospec, prob['X'], prob['y'])
    for begin, count in ((10, 16), (0, 0)):
        eng.set_row_window(begin, count)
        _check_grad(ospec, prob, slice(begin, begin + count) if count else slice(None), eng=eng, lp_tol=1e-4)


def _steps_problem():
    ospec = _ospec(1, 14, 14, 4)
    return ospec, LN.synthetic_problem(ospec, 25, 3, seed=9)


def test_pointwise_loglik_of_held_out_rows():
    ospec, prob = _steps_problem()
    test = LN.synthetic_problem(ospec, 13, 1, seed=10)
    th64 = prob['theta0'].astype(np.float64)
    _assert_off_the_kink(ospec, th64, test['X'])
    ref, _ = O.pointwise_loglik_raw(ospec, LN.forward(ospec, th64, test['X']), test['y'])
    eng = _engine(ospec, prob['X'], prob['y'])
    pw = eng.pointwise_loglik(torch.from_numpy(prob['theta0']), torch.from_numpy(test['X']), torch.from_numpy(test['y']))
    assert pw.shape == (3, 13)
    assert np.abs(pw.cpu().numpy() - ref).max() < 1e-4 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize('C,H,W,K,act,task,seed', [(1, 28, 28, 10, 'relu', 'classification', 203), (2, 13, 17, 2, 'tanh', 'regr', 3)])
def test_predict_raw_outputs(C, H, W, K, act, task, seed):
    """The bound tests/test_gpu_predict.py holds lenet_f32 to: max|out - ref| < 1e-4 max(1, max|ref|)."""
    ospec = LN.LeNetSpec(C, H, W, K, activation=act, task=task)
    prob = LN.synthetic_problem(ospec, 37, 3, seed=seed)
    th64 = prob['theta0'].astype(np.float64)
    _assert_off_the_kink(ospec, th64, prob['X'])
    out = _engine(ospec, prob['X'], prob['y']).predict(torch.from_numpy(prob['theta0']), torch.from_numpy(prob['X']))
    ref = LN.forward(ospec, th64, prob['X'])
    assert out.shape == (3, 37, K)
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref).max()
    print(f'predict {C}x{H}x{W}: {err:.2e}')
    assert err < 1e-4 * max(1.0, np.abs(ref).max()), err


def test_mclmc_steps_match_oracle():
    ospec, prob = _steps_problem()
    E, T, d = 3, 4, ospec.n_params
    _assert_off_the_kink(ospec, prob['theta0'].astype(np.float64), prob['X'])
    rng = np.random.default_rng(4)
    z0 = rng.standard_normal((E, d)).astype(np.float32)
    noise = rng.standard_normal((T, 2, E, d)).astype(np.float32)
    f = lambda th: LN.logpost_and_grad(ospec, th, prob['X'], prob['y'])
    st = O.mclmc_init(f, prob['theta0'].astype(np.float64), z0.astype(np.float64))
    for i in range(T):
        st, info = O.mclmc_step(f, st, prob['eps'].astype(np.float64), prob['L'].astype(np.float64),
                                noise[i, 0].astype(np.float64), noise[i, 1].astype(np.float64))
    eng = _engine(ospec, prob['X'], prob['y'])
    s = eng.init(torch.from_numpy(prob['theta0']), noise=torch.from_numpy(z0))
    s, info_g, _ = eng.step(s, torch.from_numpy(prob['eps']), torch.from_numpy(prob['L']), n_steps=T, noise=torch.from_numpy(noise))
    torch.cuda.synchronize()
    assert _relerr(s.position.cpu().numpy(), st.position) < 1e-4
    assert _relerr(s.logdensity.cpu().numpy(), st.logdensity) < 1e-5
    assert _relerr(s.logdensity_grad.cpu().numpy(), st.logdensity_grad) < 1e-3
    assert np.abs(info_g.energy_change[-1].cpu().numpy() - info.energy_change).max() < 5e-3


@pytest.fixture(scope='module')
def cifar8():
    """3 x 32 x 32, K = 10, N = 48, E = 8: the problem, its x3 engine and one gradient (shared, left unchanged)."""
    ospec = _ospec(3, 32, 32, 10)
    prob = LN.synthetic_problem(ospec, 48, 8, seed=0)
    eng = _engine(ospec, prob['X'], prob['y'])
    lp, g = eng.logpost_grad(torch.from_numpy(prob['theta0']))
    return ospec, prob, eng, lp.cpu(), g.cpu()


def test_deterministic_and_particles_independent(cifar8):
    ospec, prob, eng, lp, g = cifar8
    th = torch.from_numpy(prob['theta0'])
    lp2, g2 = eng.logpost_grad(th)
    assert torch.equal(lp2.cpu(), lp) and torch.equal(g2.cpu(), g)
    perm = torch.randperm(8, generator=torch.Generator().manual_seed(1))
    lp3, g3 = eng.logpost_grad(th[perm])
    assert torch.equal(lp3.cpu(), lp[perm]) and torch.equal(g3.cpu(), g[perm])


def test_image_halves_add_up(cifar8):
    ospec, prob, eng, lp, g = cifar8
    th = torch.from_numpy(prob['theta0'])
    half = lambda sl: _engine(ospec, prob['X'][sl], prob['y'][sl]).logpost_grad(th)[1].cpu()
    prior_g = -th                                       # Normal(0, 1): counted once per half
    assert _relerr((half(slice(0, 24)) + half(slice(24, 48)) - prior_g).numpy(), g.numpy()) < 5e-5


def test_agrees_with_lenet_f32(cifar8):
    """A dropped cross term shows here: bf16 operands sit at a few 1e-2, a missing second-order product at 1e-4 to 1e-3."""
    ospec, prob, eng, lp, g = cifar8
    lp2, g2 = _engine(ospec, prob['X'], prob['y'], 'lenet_f32').logpost_grad(torch.from_numpy(prob['theta0']))
    rel = ((g.double() - g2.cpu().double()).norm(dim=1) / g2.cpu().double().norm(dim=1))
    print('x3 vs lenet_f32, per particle:', rel.numpy())
    assert rel.max().item() < 1e-4, rel


def test_refusals_are_errors():
    from mile_amd import LeNetSpec
    from mile_amd._lib import MileHipError
    from mile_amd.engine import Engine
    rng = np.random.default_rng(0)
    big = Engine(LeNetSpec(1, 96, 96, 3), torch.from_numpy(rng.standard_normal((2, 96 * 96)).astype(np.float32)),
                 torch.tensor([0, 1]), device='cuda:0', grad_kernel=KERNEL)
    with pytest.raises(MileHipError, match='LDS'):
        big.logpost_grad(torch.zeros(1, big.d))
    with pytest.raises(MileHipError, match='LENET_BF16X3'):
        Engine(LeNetSpec(5, 16, 16, 3), torch.from_numpy(rng.standard_normal((2, 5 * 256)).astype(np.float32)), torch.tensor([0, 1]),
               device='cuda:0', grad_kernel=KERNEL)


def test_launch_info():
    """3 x 16 x 16 (test_gpu_parity._shape_engine's LeNet): conv2 sees 8 x 8 -> 4 x 4, ni = min(4, 57344 // (3 * 1664)) = 4.
    cm_lds_dw(CM_IN8, 8, 8, 0, ni = 4, terms = 3): planes 3 * (4 * (64 + 8) * 16 + roundup32(4 * 16) * 32) = 3 * 6656 = 19968 bytes,
    the four waves' reduction buffer 4 * (13 + 1) tiles * 64 lanes * 16 = 57344 -> 57344.
    cm_lds_dw2x(16, 16, 2, terms = 3): planes 3 * ((20 * 20 + 8) * 8 + 128 pairs * 32) = 3 * 7360 = 22080, reduction 4 * 9 * 64 * 16 = 36864.
    The report is the larger of the two kernel-gradient launches: 57344."""
    from mile_amd import LeNetSpec
    from mile_amd.engine import Engine
    rng = np.random.default_rng(0)
    eng = Engine(LeNetSpec(3, 16, 16, 4), torch.tensor(rng.standard_normal((41, 3 * 256)), dtype=torch.float32),
                 torch.tensor(rng.integers(0, 4, 41)), device='cuda:0', grad_kernel=KERNEL)
    info = eng.grad_launch_info(2)
    assert 'bf16x3' in info['kernel'] and info['block'] == 256 and info['grid'] == (1, 2)
    assert 0 < info['lds_bytes'] <= 150 * 1024
    assert info['lds_bytes'] == max(3 * (4 * 72 * 16 + 64 * 32), 4 * 14 * 64 * 16, 3 * (408 * 8 + 128 * 32), 4 * 9 * 64 * 16) == 57344

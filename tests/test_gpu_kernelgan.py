"""GPU tests (-m gpu) of kernel estimation on the esr_kgan_* kernels (csrc/esr_kgan.hip, esr_hip/kernelgan.py): the 'hip' engine against the
'stock' engine (KernelGAN/kernelGAN.py, torch.nn modules) in float64 FROM THE SAME STATE, with crops and noise injected.  Operators and
single steps are compared, never trajectories.

Bars: per tensor d(a, b) = max|a - b| / max|b|; the device result may be at most 4 x as far from float64 as the fp32
CPU 'stock' result on the same input is.  The critic's ReLU pattern is a discrete function of fp32 roundings, so the float64 (and the fp32
CPU) side runs with the DEVICE's pattern forced, the disagreements are counted and every one has to be a near-zero pre-activation (below
1e-4 of BatchNorm's unit-variance output).  Conv biases in front of a BatchNorm have an analytically zero gradient: rounding noise on all
sides, only required to be small (1e-3 of the critic's largest gradient element)."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEAD = ['first_layer.bias'] + ['feature_block.%d.bias' % i for i in (0, 3, 6, 9, 12)]
NEAR_ZERO = 1e-4


def conf_of(chan, crop=64, extra=()):
    from KernelGAN.configs import Config
    return Config().parse(['--G_chan', str(chan), '--D_chan', str(chan), '--input_crop_size', str(crop)] + list(extra))


def dist(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max())


def within(tag, hip, ref32, ref64, report):
    """The project's rule: d(hip, f64) <= 4 d(stock fp32, f64); prints the figures before it asserts."""
    dh, ds = dist(hip, ref64), dist(ref32, ref64)
    report.append((tag, dh, ds))
    print('%-40s hip %.2e  stock-fp32 %.2e' % (tag, dh, ds))
    assert dh <= 4 * ds, (tag, dh, ds)


def rand(shape, seed, lo=-1.0, hi=1.0):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * (hi - lo) + lo


def smooth(shape, seed):
    x = rand(shape, seed, 0, 1)
    x = (x + x.roll(1, -1) + x.roll(1, -2) + x.roll((1, 1), (-2, -1))) / 4
    return (x * 2 - 1).float()


def stock_pair(conf, seed):
    """Stock engines in fp64 and fp32 on the CPU with the same seeded state."""
    from KernelGAN.kernelGAN import StockEngine
    torch.manual_seed(seed)
    s32 = StockEngine(conf, 'cpu', torch.float32)
    with torch.no_grad():
        # Off the symmetric initial point: biases and BatchNorm shifts that are not 0, and a generator with positive weights whose kernel sums
        # to 0.9 — a blob like an estimated kernel — so that its output is an image of the input's size, no constraint term sits on a kink
        # and the centre of mass R / S is not a ratio of two cancelling sums (a random-sign kernel of sum 0.9 has L1 norm 100 and loses two
        # digits there on any engine).  (At xavier(0.1) the output is some 1e-5: the critic's first layer would add its bias to it, and
        # BatchNorm would then amplify the rounding of that sum a thousandfold — a state in which fp32 itself has three digits.)
        for p in s32.D.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
        for m in s32.G.layers():
            m.weight.abs_()
        s32.G.final_layer.weight.mul_(0.9 / s32.G.curr_k().sum())
    s64 = StockEngine(conf, 'cpu', torch.float64)
    s64.G.load_state_dict({k: v.double() for k, v in s32.G.state_dict().items()})
    s64.D.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in s32.D.state_dict().items()})
    return s64, s32


class ForcedReLU(nn.Module):
    """ReLU with a given activation pattern per call; records the pre-activations that disagree with it."""

    def __init__(self):
        super().__init__()
        self.masks, self.flips, self.worst, self.total = [], 0, 0.0, 0

    def forward(self, x):
        m = self.masks.pop(0).to(x.dtype).reshape(x.shape)
        bad = (x.detach() > 0) != (m > 0)
        self.flips += int(bad.sum())
        self.total += x.numel()
        if bad.any():
            self.worst = max(self.worst, float(x.detach().abs()[bad].max()))
        return x * m


def force_patterns(D, act, e):
    """Install ForcedReLUs in a stock critic; act [npass, E, 6, C, P] are the device's activations: one mask per pass and layer, in call order."""
    relus = []
    for i, m in enumerate(D.feature_block):
        if isinstance(m, (nn.ReLU, ForcedReLU)):
            D.feature_block[i] = ForcedReLU()
            relus.append(D.feature_block[i])
    for p in range(act.shape[0]):
        for l, r in enumerate(relus, start=1):
            r.masks.append((act[p, e, l] > 0).cpu())
    return relus


def flips_ok(relus):
    flips, total, worst = sum(r.flips for r in relus), sum(r.total for r in relus), max(r.worst for r in relus)
    print('ReLU pattern: %d of %d activations differ from float64, worst |pre-activation| %.2e' % (flips, total, worst))
    assert worst < NEAR_ZERO and flips <= max(2, total // 1000), (flips, total, worst)


def uv_of(D):
    return torch.cat([t.detach().double().reshape(-1) for m in D.convs() for t in (m.weight_u, m.weight_v)])


def d_grads(hip_flat, D):
    from esr_hip.kernelgan import unpack_d
    return unpack_d(hip_flat.detach().cpu(), D)


def compare_d_grads(tag, hip_flat, D64, D32, report):
    g = d_grads(hip_flat, D64)
    p64, p32 = dict(D64.named_parameters()), dict(D32.named_parameters())
    gmax = max(float(p.grad.abs().max()) for p in p64.values())
    for n in p64:
        if n in DEAD:
            assert float(g[n].abs().max()) < 1e-3 * gmax, (tag, n)
        else:
            within('%s d/d %s' % (tag, n), g[n], p32[n].grad, p64[n].grad, report)


# ---- the generator as one kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,E', [(8, 1), (8, 3), (64, 1), (64, 3)])
def test_compose_and_adjoint(C, E):
    from esr_hip.kernelgan import KernelGanEngine
    conf = conf_of(C)
    eng = KernelGanEngine(E, conf)
    pairs = [stock_pair(conf, 10 + e) for e in range(E)]
    for e, (s64, s32) in enumerate(pairs):
        eng.load_stock(e, s32.G, s32.D)
    k = eng.curr_k()
    cot = rand((E, 13, 13), 5).float().cuda().contiguous()
    eng._compose_bwd(cot)
    report = []
    for e, (s64, s32) in enumerate(pairs):
        ks = []
        for s in (s64, s32):
            kk = s.G.curr_k()
            (kk * cot[e].cpu().to(kk.dtype)).sum().backward()
            ks.append(kk)
        within('k[%d]' % e, k[e], ks[1], ks[0], report)
        for l, (m64, m32) in enumerate(zip(s64.G.layers(), s32.G.layers())):
            within('d/dw%d[%d]' % (l, e), eng.gw[l].grad[e], m32.weight.grad, m64.weight.grad, report)


def kernel_like(E, seed):
    yy, xx = np.mgrid[:13, :13]
    ks = []
    for e in range(E):
        k = np.exp(-((yy - 5.4 - e) ** 2 / (5.0 + e) + (xx - 6.8) ** 2 / 2.5 + 0.3 * (yy - 5.4) * (xx - 6.8)))
        ks.append(k / k.sum() * (1.05 - 0.1 * e))
    return torch.as_tensor(np.stack(ks)) + 0.003 * rand((E, 13, 13), seed)


@pytest.mark.parametrize('H,W', [(16, 18), (64, 64)])
def test_apply_k_bicubic_term_constraints_and_dk(H, W):
    """y, the bicubic downscale, every loss term and dL/dk (data term through an injected dL/dy, lambda-weighted constraints with the centralized and
    sparse terms switched on) against autograd through the stock engine's formulas in float64.  The 16 x 18 crop has 2 x 3 outputs."""
    from esr_hip.kernelgan import KernelGanEngine
    E, conf = 2, conf_of(8)
    eng = KernelGanEngine(E, conf)
    s64, s32 = stock_pair(conf, 3)
    lambdas = dict(bicubic=0.05, sum2one=0.5, boundaries=0.5, centralized=1., sparse=5.)
    for d in eng.lambdas:
        d.update(lambdas)
    eng.push_lambdas()
    x, k = smooth((E, 3, H, W), 21), kernel_like(E, 22).float()
    oh, ow = (H - 12) // 2, (W - 12) // 2
    dgan = rand((E, 3, oh, ow), 23).float() * 1e-3
    xg, kg, dg = x.cuda().contiguous(), k.cuda().contiguous(), dgan.cuda().contiguous()
    b = eng.apply_k(xg, kg)
    assert b.y.shape == (E, 3, oh, ow)
    eng.dk_from(xg, dg)
    dk_data = b.dk.clone()
    eng.constraints(kg, b)
    report = []
    for e in range(E):
        res = []
        for s in (s64, s32):
            s.lambdas = dict(lambdas)
            ke = k[e].to(s.dtype).clone().requires_grad_(True)
            xe = x[e:e + 1].to(s.dtype)
            y = F.conv2d(xe.transpose(0, 1), ke[None, None], stride=2).transpose(0, 1)
            bic = s.bicubic_downscale(xe, y)
            losses = s.constraint_losses(xe, y, ke)
            data = (y * dgan[e:e + 1].to(s.dtype)).sum() + lambdas['bicubic'] * losses['bicubic']
            gd, = torch.autograd.grad(data, ke, retain_graph=True)
            gt, = torch.autograd.grad(data + sum(lambdas[n] * losses[n] for n in lambdas if n != 'bicubic'), ke)
            res.append((y, bic, losses, gd, gt))
        (y64, bic64, l64, gd64, gt64), (y32, bic32, l32, gd32, gt32) = res
        within('y[%d]' % e, b.y[e], y32[0], y64[0], report)
        within('bic[%d]' % e, b.bic[e], bic32[0, 0], bic64[0, 0], report)
        assert dist(bic64[0, 0], bic64[0, 2]) == 0                           # upstream's quirk: every plane is the sum over the three input planes
        names = ('bicubic', 'sum2one', 'boundaries', 'centralized', 'sparse')
        within('the five losses[%d]' % e, eng.losses[e], torch.stack([l32[n] for n in names]), torch.stack([l64[n] for n in names]), report)
        within('dk data[%d]' % e, dk_data[e], gd32, gd64, report)
        within('dk total[%d]' % e, b.dk[e], gt32, gt64, report)


def test_crop_gather_from_resident_images():
    """Crops of two images of different sizes, even corners, one at the image's far corner; with and without noise.  out = 2 (img + noise / 255) - 1 in
    fp32: the same three operations as NumPy's, so at most one rounding apart (2^-23 at values up to 2)."""
    from esr_hip.kernelgan import KernelGanEngine
    eng = KernelGanEngine(2, conf_of(8))
    rng = np.random.RandomState(4)
    images = [rng.rand(70, 66, 3).astype(np.float32), rng.rand(64, 90, 3).astype(np.float32)]
    corners = np.array([[[4, 2, 44, 40], [0, 26, 38, 64]], [[6, 0, 0, 0], [0, 0, 10, 12]]], dtype=np.int32)
    eng.set_images(images, corners)
    noise = torch.randn(2, 3, 26, 26, generator=torch.Generator().manual_seed(1))
    b = eng._gb(64, 64)
    from esr_hip._lib import lib as L
    for it in range(2):
        assert L.esr_kgan_gather(eng.imgs.data_ptr(), eng.meta.data_ptr(), eng.tl_g[it].data_ptr(), None, eng.g_in.data_ptr(), 2, 64, None) == 0
        assert L.esr_kgan_gather(eng.imgs.data_ptr(), eng.meta.data_ptr(), eng.tl_d[it].data_ptr(), noise.cuda().data_ptr(), b.xin[0].data_ptr(), 2, 26, None) == 0
        torch.cuda.synchronize()
        for e in range(2):
            tg, lg, td, ld = corners[it, e]
            ref_g = np.transpose(images[e][tg:tg + 64, lg:lg + 64], (2, 0, 1)) * np.float32(2) - np.float32(1)
            ref_d = (np.transpose(images[e][td:td + 26, ld:ld + 26], (2, 0, 1)) + noise[e].numpy() / np.float32(255)) * np.float32(2) - np.float32(1)
            assert np.abs(eng.g_in[e].cpu().numpy() - ref_g).max() <= 2.0 ** -23
            assert np.abs(b.xin[0, e].cpu().numpy() - ref_d).max() <= 2.0 ** -22
    from esr_hip import EsrError
    bad = corners.copy()
    bad[1, 0, 0] = 8                                            # 8 + 64 > 70 rows
    with pytest.raises(EsrError, match='leaves the image'):
        eng.set_images(images, bad)


# ---- the critic ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [8, 64])
@pytest.mark.parametrize('H,W', [(10, 12), (26, 26)])
def test_critic_two_forwards_parameter_gradients_and_data_gradient(C, H, W):
    """A D step's two forwards (real against 1, fake against 0, half their sum; the second power iteration starts from the first's u), then a G step's
    single forward with its data gradient — 24 positions (less than one wave) and 400 (a ragged last wave)."""
    from esr_hip.kernelgan import KernelGanEngine
    E, conf = 2, conf_of(C)
    eng = KernelGanEngine(E, conf)
    pairs = [stock_pair(conf, 40 + e) for e in range(E)]
    for e, (s64, s32) in enumerate(pairs):
        eng.load_stock(e, s32.G, s32.D)
    x = smooth((2, E, 3, H, W), 31)
    c = eng.critic(x.cuda().contiguous(), (1., 0.), 0.5, True, False)
    report = []
    for e, (s64, s32) in enumerate(pairs):
        outs = []
        for s in (s64, s32):
            relus = force_patterns(s.D, c.act, e)
            real, fake = s.D(x[0, e:e + 1].to(s.dtype)), s.D(x[1, e:e + 1].to(s.dtype))
            l_real, l_fake = (real - 1).abs().mean(), fake.abs().mean()
            ((l_real + l_fake) * 0.5).backward()
            outs.append((real, fake, l_real, l_fake))
            if s is s64:
                flips_ok(relus)
        (r64, f64, lr64, lf64), (r32, f32, lr32, lf32) = outs
        within('pred real[%d]' % e, c.pred[0, e], r32[0, 0], r64[0, 0], report)
        within('pred fake[%d]' % e, c.pred[1, e], f32[0, 0], f64[0, 0], report)
        within('losses real, fake[%d]' % e, c.loss[:, e], torch.stack((lr32, lf32)), torch.stack((lr64, lf64)), report)
        compare_d_grads('D step [%d]' % e, eng.dp.grad[e], s64.D, s32.D, report)
        within('u, v after two forwards[%d]' % e, eng.uv[e], uv_of(s32.D), uv_of(s64.D), report)
    # the G step's use: one forward against 1, the gradient at the input (a third power iteration from the state the two above left)
    y = smooth((1, E, 3, H, W), 32)
    c1 = eng.critic(y.cuda().contiguous(), (1.,), 1., False, True)
    for e, (s64, s32) in enumerate(pairs):
        gs = []
        for s in (s64, s32):
            relus = force_patterns(s.D, c1.act, e)
            ye = y[0, e:e + 1].to(s.dtype).clone().requires_grad_(True)
            (s.D(ye) - 1).abs().mean().backward()
            gs.append(ye.grad)
            if s is s64:
                flips_ok(relus)
        within('d/dx[%d]' % e, c1.dx[0, e], gs[1][0], gs[0][0], report)


# ---- one iteration ------------------------------------------------------------------------------------------------------------------
def test_one_full_step_at_the_default_shape():
    """step() = G step then D step at 64 channels and 64 x 64 crops with lambda_centralized = 1 and lambda_sparse = 5.  The stock engines take the
    device's updated generator before their D step, so both halves start from identical states."""
    from esr_hip.kernelgan import KernelGanEngine
    conf = conf_of(64)
    eng = KernelGanEngine(1, conf)
    s64, s32 = stock_pair(conf, 77)
    eng.load_stock(0, s32.G, s32.D)
    lambdas = dict(bicubic=5e-4, sum2one=0.5, boundaries=0.5, centralized=1., sparse=5.)
    eng.lambdas[0].update(lambdas)
    eng.push_lambdas()
    g_in, d_in, noise = smooth((1, 3, 64, 64), 51), smooth((1, 3, 26, 26), 52), torch.randn(1, 3, 26, 26, generator=torch.Generator().manual_seed(53))
    before = [p.detach().clone() for p in eng.gw] + [eng.dp.detach().clone()]
    eng.step(g_in.cuda(), d_in.cuda(), noise.cuda(), slot=7)
    torch.cuda.synchronize()
    report = []
    cg, cd = eng._critic_bufs[(1, 26, 26)], eng._critic_bufs[(2, 26, 26)]
    for s in (s64, s32):
        s.lambdas = dict(lambdas)
        relus = force_patterns(s.D, cg.act, 0)
        s.train_g(g_in.to(s.dtype), update=False)
        if s is s64:
            flips_ok(relus)
    names = ('bicubic', 'sum2one', 'boundaries', 'centralized', 'sparse')
    within('the G step\'s six losses', torch.cat((eng.loss_g[:1], eng.losses[0])), torch.stack([s32.loss_g] + [s32.losses[n] for n in names]),
           torch.stack([s64.loss_g] + [s64.losses[n] for n in names]), report)
    assert float(eng.bic_log[0, 7]) == float(eng.losses[0, 0]) and float(eng.bic_log[0].abs().sum()) == float(eng.losses[0, 0])
    for l, (m64, m32) in enumerate(zip(s64.G.layers(), s32.G.layers())):
        within('G step d/dw%d' % l, eng.gw[l].grad[0], m32.weight.grad, m64.weight.grad, report)
    for s in (s64, s32):
        with torch.no_grad():
            for l, m in enumerate(s.G.layers()):
                m.weight.copy_(eng.gw[l][0].detach().cpu().to(s.dtype))
        relus = force_patterns(s.D, cd.act, 0)
        s.train_d(g_in.to(s.dtype), d_in.to(s.dtype), noise.to(s.dtype), update=False)
        if s is s64:
            flips_ok(relus)
    within('loss_d real, fake', eng.loss_d[:, 0], torch.stack((s32.loss_d_real, s32.loss_d_fake)), torch.stack((s64.loss_d_real, s64.loss_d_fake)), report)
    compare_d_grads('D step', eng.dp.grad[0], s64.D, s32.D, report)
    # Adam moved every parameter, by at most lr at its first step
    for p0, p in zip(before, eng.gw + [eng.dp]):
        step = (p.detach() - p0).abs()
        # lr, up to esr_adam_run's fp32 betas (1 - 0.999f is 1.3e-5 off 0.001: 6e-6 of the step) and one rounding of the parameter
        assert float(step.max()) <= 2e-4 * (1 + 1e-4) + 2.0 ** -23 * float(p0.abs().max()) and float(step.max()) > 1e-4


def run_steps(E, states, conf, seeds, n=2):
    from esr_hip.kernelgan import KernelGanEngine
    eng = KernelGanEngine(E, conf)
    for e, (G, D) in enumerate(states):
        eng.load_stock(e, G, D)
    for i in range(n):
        g_in = torch.cat([smooth((1, 3, 64, 64), 100 * s + i) for s in seeds]).cuda()
        d_in = torch.cat([smooth((1, 3, 26, 26), 100 * s + 10 + i) for s in seeds]).cuda()
        noise = torch.cat([rand((1, 3, 26, 26), 100 * s + 20 + i).float() for s in seeds]).cuda()
        eng.step(g_in, d_in, noise, slot=i)
    torch.cuda.synchronize()
    return [p.detach().cpu() for p in eng.gw] + [eng.dp.detach().cpu(), eng.uv.cpu(), eng.bic_log.cpu()[:, :n]]


def test_batched_estimations_equal_single_ones_bit_for_bit_and_runs_repeat():
    conf = conf_of(8)
    states = []
    for e in range(3):
        _, s32 = stock_pair(conf, 60 + e)
        states.append((s32.G, s32.D))
    a = run_steps(3, states, conf, (1, 2, 3))
    b = run_steps(3, states, conf, (1, 2, 3))
    for ta, tb in zip(a, b):
        assert torch.equal(ta, tb)
    for e in range(3):
        one = run_steps(1, states[e:e + 1], conf, (e + 1,))
        for t3, t1 in zip(a, one):
            assert torch.equal(t3[e], t1[0]), e


def synthetic_image(seed, kernel_sigma):
    rng = np.random.RandomState(seed)
    big = rng.rand(42, 36, 3)
    big = np.kron(big, np.ones((5, 5, 1)))[:192 + 12, :160 + 12]
    ax = np.arange(-6, 7)
    g = np.exp(-ax ** 2 / (2 * kernel_sigma ** 2))
    g /= g.sum()
    blur = np.apply_along_axis(lambda r: np.convolve(r, g, 'valid'), 0, big)
    blur = np.apply_along_axis(lambda r: np.convolve(r, g, 'valid'), 1, blur)
    return np.clip(blur[::2, ::2] * 255, 0, 255).astype(np.uint8)


def test_train_batch_end_to_end_and_the_cem_of_the_result():
    """Two 96 x 80 images, 300 iterations in lock step: sane kernels (finite, non-negative up to the shift's spline ripple, sum 1, centre of mass where kernel_shift puts it), and
    create_model builds its CEM from one."""
    from scipy.ndimage import center_of_mass
    from KernelGAN import train as KernelGAN
    from KernelGAN import util
    images = [synthetic_image(1, 1.2), synthetic_image(2, 2.0)]
    assert images[0].shape == (96, 80, 3)
    confs = []
    for im in images:
        conf = KernelGAN.Config().parse(['--X4', '--real_image', '--max_iters', '300'])
        conf.LR_image = im
        confs.append(conf)
    torch.manual_seed(0)
    np.random.seed(0)
    ks = KernelGAN.train_batch(confs)
    assert len(ks) == 2 and not np.array_equal(ks[0], ks[1])
    for k in ks:
        assert k.ndim == 2 and k.shape[0] == k.shape[1] and np.isfinite(k).all()
        # Non-negative up to what the reference's own post-processing does: its kernel_shift moves the clipped, non-negative kernel with an
        # interpolating cubic spline, whose side lobes undershoot by at most 0.13 of a peak (the recorded reference result in
        # tests/golden/kernelgan.npz has -1e-3 there); nothing else may go below zero.
        assert k.min() >= -0.13 * k.max() and abs(k.sum() - 1) < 1e-9
        # the x2 kernel (odd side n, centre of mass c + 0.5) squares to centre of mass 3 (c + 0.5) - n // 2 = the x4 target, centre + 1.5;
        # the spline shift leaves the x2 one within 0.05 of its target (tests/test_host_kernelgan.py), three times that here
        assert np.abs(np.array(center_of_mass(k)) - util.wanted_center(k.shape, 4)).max() < 0.15
    conf2 = KernelGAN.Config().parse(['--real_image', '--max_iters', '20'])
    conf2.LR_image = images[0]
    k2 = KernelGAN.train(conf2)
    assert np.abs(np.array(center_of_mass(k2)) - util.wanted_center(k2.shape, 2)).max() < 0.05
    import models
    from test_gpu_callers_f7 import product_opt
    opt = product_opt(False)
    opt['test']['kernel'] = 'estimated'
    from CEM.imresize_CEM import imresize
    imresize.kernels = {}
    try:
        m = models.create_model(opt, kernel=ks[0])
        assert m.CEM_net is not None
        assert imresize.kernels['4'].shape[0] > 17                 # the CEM was built from the estimated kernel, not from the 16-tap bicubic one
    finally:
        imresize.kernels = {}           # a custom kernel replaces the x4 kernel PROCESS-WIDE (as in the reference): do not leave it to the next test

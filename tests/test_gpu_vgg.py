"""GPU tests (-m gpu) of the VGG feature extractor on the library's kernels (esr_hip/vgg.py, csrc/esr_vgg.hip; reference
codes/models/modules/architecture.py:658-705 over torchvision's VGG `features`, the feature loss of codes/models/SRRaGAN_model.py:442-451 and
the Z objectives 'VGG' / 'max_VGG' of codes/Z_optimization.py:505-507,729-731).

The oracle is an fp64 torch-CPU restatement (F.conv2d / relu / max_pool2d) on the same seeded weights (torchvision's init: kaiming normal,
fan-out).  Gradients are compared flip-proof, as tests/test_gpu_backward.py does for the generator: the ReLU pattern and the pool argmax the
GPU forward took (read from the activations it kept) are forced onto the oracle, so what remains between the two is arithmetic error."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.check_golden import rel_l2
from oracle.weights import seeded_uniform
from test_host_vgg import seeded_state_dict

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
# 'bf16' bar: one bf16 rounding (2^-9 relative, rms ~2^-9/sqrt(3)) of each operand of every product, 16 conv layers whose errors add up
# like a random walk: sqrt(16 * 2) * 2^-9 / sqrt(3) ~ 6e-3 for the features; 3e-2 leaves a factor ~5 for ReLU / argmax flips and
# error growth through the net.  The same for the input gradient, which goes back through the same 16 layers.
BF16_BAR = 3e-2
SPLIT_BAR = 1e-3          # the generator tests' relative bar


def vgg19(feature_layer=34, seed=0):
    import models.modules.architecture as arch
    sd = seeded_state_dict('vgg19', feature_layer, seed=seed, extra=False)
    return arch.VGGFeatureExtractor(feature_layer=feature_layer, state_dict=sd).to(DEV).eval(), sd


def oracle(sd, features, x, mean, std, masks=None, argmax=None):
    """fp64 features of x (CPU).  masks / argmax: per ReLU the GPU's pattern (stored output > 0) and per pool its window argmax (flat
    indices of F.max_pool2d(return_indices=True)) forced instead of taking them from the oracle's own values."""
    y = (x.double() - mean.double()) / std.double()
    ri = pi = 0
    for i, m in enumerate(features):
        if isinstance(m, torch.nn.Conv2d):
            y = F.conv2d(y, sd['features.%d.weight' % i].double(), sd['features.%d.bias' % i].double(), padding=1)
        elif isinstance(m, torch.nn.ReLU):
            y = y * masks[ri].double() if masks is not None else F.relu(y)
            ri += 1
        else:
            if argmax is None:
                y = F.max_pool2d(y, 2)
            else:
                idx = argmax[pi]
                B, Cc, h, w = idx.shape
                y = y.flatten(2).gather(2, idx.flatten(2)).view(B, Cc, h, w)
            pi += 1
    return y


def gpu_pattern(net, saved):
    """(ReLU masks, pool argmax) of the GPU forward, from the activations the engine kept (saved = the autograd node's `saved`)."""
    _, outs = saved
    ops = net.engine.ops
    masks = [(_unpack(t, op.cout) > 0).cpu() for op, t in zip(ops, outs) if op.kind == 'conv' and op.relu]
    argmax = [F.max_pool2d(_unpack(outs[j - 1], ops[j - 1].cout).cpu(), 2, return_indices=True)[1] for j, op in enumerate(ops) if op.kind == 'pool']
    return masks, argmax


def _unpack(t, nc):
    from esr_hip import _lib
    from esr_hip.act import view_of
    B = t.shape[1]
    out = torch.empty(B, nc, t.shape[3] - 2, t.shape[4] - 2, dtype=torch.float32, device=t.device)
    assert _lib.lib.esr_unpack_nchw(C.byref(view_of(t)), B, nc, out.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    return out


def _pack(x, planes):
    """fp32 NCHW (GPU) -> activation tensor [planes][B][CG][H+2][W+2][8] (no normalisation)."""
    from esr_hip import _lib
    from esr_hip.act import new_at, view_of
    B, Cc, H, W = x.shape
    t = new_at(planes, B, (Cc + 7) // 8, H, W, x.device)
    assert _lib.lib.esr_pack_nchw_norm(x.data_ptr(), B, Cc, H, W, None, None, C.byref(view_of(t)), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    return t


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize('precision', ['split', 'bf16'])
def test_relu_conv_and_its_masked_data_gradient(precision):
    """conv(3 -> 64) + ReLU (act_slope 0) -> conv(64 -> 64): forward against fp64, and the input gradient, whose second data-gradient launch
    applies ReLU's backward as its mask (mask_slope 0)."""
    import models.modules.architecture as arch
    g = torch.Generator().manual_seed(11)
    sd = {'features.0.weight': torch.randn(64, 3, 3, 3, generator=g) * 0.2, 'features.0.bias': torch.randn(64, generator=g) * 0.1,
          'features.2.weight': torch.randn(64, 64, 3, 3, generator=g) * 0.06, 'features.2.bias': torch.randn(64, generator=g) * 0.1}
    net = arch.VGGFeatureExtractor(feature_layer=2, state_dict=sd, use_input_norm=False).to(DEV).eval()
    net.set_precision(precision)
    x = seeded_uniform((2, 3, 23, 30), 12, -1.0, 1.0)
    xg = x.to(DEV).requires_grad_(True)
    feat = net(xg)
    saved = feat.grad_fn.saved
    masks, _ = gpu_pattern(net, saved)
    assert 0.2 < float(masks[0].float().mean()) < 0.8                      # the ReLU does cut
    ref = oracle(sd, net.features, x, torch.zeros(1, 3, 1, 1), torch.ones(1, 3, 1, 1))
    bar = SPLIT_BAR if precision == 'split' else BF16_BAR
    assert rel_l2(feat.detach().cpu().double(), ref) < bar / 3
    cot = seeded_uniform(tuple(feat.shape), 13, -1.0, 1.0)
    (feat * cot.to(DEV)).sum().backward()
    xo = x.double().requires_grad_(True)
    (oracle(sd, net.features, xo, torch.zeros(1, 3, 1, 1), torch.ones(1, 3, 1, 1), masks=masks) * cot.double()).sum().backward()
    assert rel_l2(xg.grad.cpu().double(), xo.grad) < bar / 3


@pytest.mark.parametrize('precision', ['split', 'bf16'])
@pytest.mark.parametrize('shape', [(2, 16, 10, 12), (1, 24, 9, 7)], ids=['even', 'odd'])
def test_maxpool_forward_backward(precision, shape):
    """esr_maxpool2x2 copies the window maximum (hi and lo bit for bit, torch's argmax); esr_maxpool2x2_grad scatters dy to that argmax,
    with and without the fused ReLU backward.  Against F.max_pool2d on the values the activation tensor holds: exact."""
    from esr_hip import _lib
    from esr_hip.act import new_at, view_of
    P = 2 if precision == 'split' else 1
    B, Cc, H, W = shape
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = seeded_uniform(shape, 21, -1.0, 1.0)
    xt = _pack(x.to(DEV), P)
    xv = _unpack(xt, Cc).cpu()                            # what the kernels see (hi + lo)
    y = new_at(P, B, xt.shape[2], H // 2, W // 2, DEV)
    assert _lib.lib.esr_maxpool2x2(C.byref(view_of(xt)), C.byref(view_of(y)), B, s) == 0
    assert torch.equal(_unpack(y, Cc).cpu(), F.max_pool2d(xv, 2))
    assert float(y[:, :, :, 0].float().abs().max()) == 0 and float(y[:, :, :, :, -1].float().abs().max()) == 0      # border written
    dy = seeded_uniform((B, Cc, H // 2, W // 2), 22, -1.0, 1.0)
    dyt = _pack(dy.to(DEV), P)
    dyv = _unpack(dyt, Cc).cpu()
    for relu in (0, 1):
        dx = new_at(P, B, xt.shape[2], H, W, DEV)
        assert _lib.lib.esr_maxpool2x2_grad(C.byref(view_of(xt)), C.byref(view_of(dyt)), relu, C.byref(view_of(dx)), B, s) == 0
        xr = xv.clone().requires_grad_(True)
        F.max_pool2d(xr, 2).backward(dyv)
        want = xr.grad * (xv > 0) if relu else xr.grad
        assert torch.equal(_unpack(dx, Cc).cpu(), want), relu
        assert float(dx[:, :, :, 0].float().abs().max()) == 0 and float(dx[:, :, :, -1].float().abs().max()) == 0


@pytest.mark.parametrize('precision', ['split', 'bf16'])
def test_maxpool_exact_ties_and_nan_follow_torch(precision):
    """Windows full of exact ties (values from {0, 1, 2}): the first maximum in row-major order wins, as in torch; a NaN propagates."""
    from esr_hip import _lib
    from esr_hip.act import new_at, view_of
    P = 2 if precision == 'split' else 1
    B, Cc, H, W = 2, 8, 8, 10
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = torch.randint(0, 3, (B, Cc, H, W), generator=torch.Generator().manual_seed(31)).float()
    x[0, 0, 0, 1] = float('nan')                              # one NaN in window (0, 0) of image 0 channel 0
    xt = _pack(x.to(DEV), P)
    y = new_at(P, B, 1, H // 2, W // 2, DEV)
    assert _lib.lib.esr_maxpool2x2(C.byref(view_of(xt)), C.byref(view_of(y)), B, s) == 0
    yv, want = _unpack(y, Cc).cpu(), F.max_pool2d(x, 2)
    assert torch.isnan(yv[0, 0, 0, 0]) and torch.equal(torch.nan_to_num(yv, 7.0), torch.nan_to_num(want, 7.0))
    dy = torch.arange(1, B * Cc * (H // 2) * (W // 2) + 1, dtype=torch.float32).view(B, Cc, H // 2, W // 2)
    dyt = _pack(dy.to(DEV), P)
    dx = new_at(P, B, 1, H, W, DEV)
    assert _lib.lib.esr_maxpool2x2_grad(C.byref(view_of(xt)), C.byref(view_of(dyt)), 0, C.byref(view_of(dx)), B, s) == 0
    xr = x.clone().requires_grad_(True)
    F.max_pool2d(xr, 2).backward(_unpack(dyt, Cc).cpu())
    assert torch.equal(_unpack(dx, Cc).cpu(), xr.grad)


# ------------------------------------------------------------------------------------------------ the extractor
@pytest.mark.parametrize('precision', ['split', 'bf16'])
@pytest.mark.parametrize('shape', [(2, 3, 208, 208), (1, 3, 100, 75)], ids=['2x208', '1x100x75'])
def test_vgg19_features_and_input_gradient(precision, shape):
    net, sd = vgg19(seed=5)
    net.set_precision(precision)
    x = seeded_uniform(shape, 41)
    xg = x.to(DEV).requires_grad_(True)
    feat = net(xg)
    assert feat.shape == (shape[0], 512, shape[2] // 16, shape[3] // 16)
    bar = SPLIT_BAR if precision == 'split' else BF16_BAR
    ref = oracle(sd, net.features, x, net.mean.cpu(), net.std.cpu())
    err = rel_l2(feat.detach().cpu().double(), ref)
    assert err < bar, err
    # no-graph pass: the same features
    with torch.no_grad():
        assert torch.equal(net(x.to(DEV)), feat.detach())
    saved = feat.grad_fn.saved
    masks, argmax = gpu_pattern(net, saved)
    cot = seeded_uniform(tuple(feat.shape), 42, -1.0, 1.0)
    (feat * cot.to(DEV)).sum().backward()
    xo = x.double().requires_grad_(True)
    (oracle(sd, net.features, xo, net.mean.cpu(), net.std.cpu(), masks=masks, argmax=argmax) * cot.double()).sum().backward()
    gerr = rel_l2(xg.grad.cpu().double(), xo.grad)
    assert gerr < bar, gerr
    assert all(p.grad is None for p in net.parameters())


# ------------------------------------------------------------------------------------------------ the model and the Z search
def _esrgan_opt(tmp_path, cem, wpath):
    from test_host_api import _opt
    opt = _opt(nb=1, lat=0, cem=cem, is_train=True)
    opt['gpu_ids'] = [0]
    opt['path']['models'] = str(tmp_path / 'models')
    opt['path']['log'] = str(tmp_path / 'log')
    opt['path']['pretrained_model_F'] = wpath
    # train_esrgan.json's losses on the generator side: l1 pixel loss (1e-2) and the l1 VGG19-54 feature loss (weight 1)
    opt['train']['pixel_weight'] = 1e-2
    opt['train']['feature_weight'] = 1
    opt['train']['feature_criterion'] = 'l1'
    return opt


def _weights_file(tmp_path):
    p = str(tmp_path / 'vgg19_tv.pth')
    torch.save(seeded_state_dict('vgg19', 34, seed=7), p)
    return p


def _make_model(tmp_path, cem, use_plans=True):
    import models
    from oracle.weights import fill_formula_weights
    m = models.create_model(_esrgan_opt(tmp_path, cem, _weights_file(tmp_path)))
    fill_formula_weights(m.netG, gain=1.0)
    eng = m.netG.generated_image_model.engine if cem else m.netG.engine
    eng.use_plans = use_plans
    return m


@pytest.mark.parametrize('cem', [False, True], ids=['plain', 'cem'])
def test_srragan_feature_loss_matches_oracle(tmp_path, cem):
    m = _make_model(tmp_path, cem)
    lr = seeded_uniform((2, 3, 24, 26), 51)
    hr = seeded_uniform((2, 3, 96, 104), 52)
    for _ in range(2):                       # without a critic the first call is idle (reference SRRaGAN_model.py:338-339)
        m.feed_data({'LR': lr, 'HR': hr})
        m.optimize_parameters()
    l_fea = m.get_current_log()['l_g_fea']
    sd = {k: v.detach().cpu() for k, v in m.netF.state_dict().items()}
    fake, real = m.fake_H.detach().cpu(), m.var_H.detach().cpu()
    mean, std = m.netF.mean.cpu(), m.netF.std.cpu()
    ref = (oracle(sd, m.netF.features, fake, mean, std) - oracle(sd, m.netF.features, real, mean, std)).abs().mean().item()
    assert abs(l_fea - ref) < SPLIT_BAR * abs(ref), (l_fea, ref)
    # the gradient the feature term sends into fake_H (the same calls the G step makes)
    fh = m.fake_H.detach().clone().requires_grad_(True)
    with torch.no_grad():
        real_fea = m.netF(m.var_H)
    fake_fea = m.netF(fh)
    masks, argmax = gpu_pattern(m.netF, fake_fea.grad_fn.saved)
    m.cri_fea(fake_fea, real_fea).backward()
    fo = fake.double().requires_grad_(True)
    # (the sign of L1's gradient is taken where the GPU's features differ: both sides see the same sign pattern)
    diff_sign = torch.sign(fake_fea.detach().cpu().double() - real_fea.cpu().double())
    fo_fea = oracle(sd, m.netF.features, fo, mean, std, masks=masks, argmax=argmax)
    (fo_fea * diff_sign).sum().div(diff_sign.numel()).backward()
    assert rel_l2(fh.grad.cpu().double(), fo.grad) < SPLIT_BAR
    assert all(p.grad is None for p in m.netF.parameters())


def test_srragan_steps_with_recorded_passes_match_eager(tmp_path):
    """Two consecutive G steps with the generator's recorded launch lists (default) and with every launch issued from Python: same results."""
    res = []
    for use_plans in (True, False):
        torch.manual_seed(0)
        m = _make_model(tmp_path, True, use_plans=use_plans)
        lr = seeded_uniform((2, 3, 24, 26), 61)
        hr = seeded_uniform((2, 3, 96, 104), 62)
        for _ in range(3):
            m.feed_data({'LR': lr, 'HR': hr})
            m.optimize_parameters()
        log = m.log_dict
        res.append(([v for _, v in log['l_g_fea']], m.fake_H.detach().cpu(), torch.cat([p.detach().reshape(-1).cpu() for p in m.netG.parameters()])))
    (la, fa, pa), (lb, fb, pb) = res
    assert len(la) == 2 and len(lb) == 2
    np.testing.assert_allclose(la, lb, rtol=1e-6)
    assert torch.allclose(fa, fb, rtol=0, atol=1e-6) and torch.allclose(pa, pb, rtol=0, atol=1e-7)


@pytest.mark.parametrize('objective', ['VGG', 'max_VGG'])
def test_z_optimizer_vgg_objectives(tmp_path, objective):
    import models
    from test_host_api import _opt
    from Z_optimization import Z_optimizer
    from oracle.weights import fill_formula_weights
    lat, B = 3, 1
    opt = _opt(nb=1, lat=lat, cem=True, is_train=False)
    opt['gpu_ids'] = [0]
    opt['path']['pretrained_model_F'] = _weights_file(tmp_path)
    m = models.create_model(opt, init_Fnet=True)
    fill_formula_weights(m.netG, gain=1.0)
    assert not m.netF.training
    lr = seeded_uniform((1, 3, 16, 16), 71)
    z0 = seeded_uniform((B, lat, 64, 64), 72, -0.5, 0.5)
    m.feed_data({'LR': lr.to(DEV), 'Z': z0.to(DEV)}, need_GT=False)
    m.test()
    desired = seeded_uniform((B, 3, 64, 64), 73)
    zo = Z_optimizer(objective=objective, Z_size=[64, 64], model=m, Z_range=1, max_iters=6, data={'LR': lr.to(DEV), 'desired': desired.to(DEV)},
                     initial_LR=0.05, batch_size=B, initial_Z=z0.to(DEV))
    zo.optimize()
    vals = zo.loss_values
    assert len(vals) >= 1
    with pytest.raises(NotImplementedError):
        Z_optimizer(objective=objective, Z_size=[64, 64], model=m, Z_range=1, max_iters=1, initial_LR=0.05, image_mask=np.ones((64, 64)),
                    Z_mask=np.ones((64, 64)))

    def vgg_distance():
        m.feed_data({'LR': lr.to(DEV), 'Z': zo.Z_model().detach()}, need_GT=False)
        m.test()
        with torch.no_grad():
            return float((m.netF(m.Output_Batch(within_0_1=True)) - m.netF(desired.to(DEV))).abs().mean())
    m.feed_data({'LR': lr.to(DEV), 'Z': z0.to(DEV)}, need_GT=False)
    m.test()
    with torch.no_grad():
        d0 = float((m.netF(m.Output_Batch(within_0_1=True)) - m.netF(desired.to(DEV))).abs().mean())
    d1 = vgg_distance()
    if objective == 'VGG':
        assert d1 < d0 * 0.999, (d0, d1)
    else:
        assert d1 > d0 * 1.001, (d0, d1)

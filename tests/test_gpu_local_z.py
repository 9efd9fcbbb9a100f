"""GPU tests (-m gpu) of the local-STD and periodicity Z objectives (csrc/esr_local.hip through esr_hip/local.py; reference
codes/Z_optimization.py:391-398, 459-509, 616-627, 799-815):
  * the patch-STD kernels against a float64 restatement (value, gradient), flat windows, determinism, batch independence;
  * the shifted-L1 kernels against float64 grid_sample / crops (integer and non-integer, 1 and 2 points, non-square, masked);
  * the reference's own values (tests/golden/local_z.npz, tools/gen_local_z_golden.py): function level (a) and Z_optimizer.optimize() runs on
    the F7 model (b).
The CPU fallbacks of esr_hip.local are patched to raise for every test here: what is graded is the kernels."""
import atexit
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch

from oracle.weights import fill_formula_weights, seeded_uniform
from oracle.zobj_contract_ref import shift64, std64

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'local_z.npz')
RUN_DIR = tempfile.mkdtemp(prefix='esr_local_z_')
atexit.register(shutil.rmtree, RUN_DIR, True)
DEV = 'cuda'


@pytest.fixture(autouse=True)
def kernels_only(monkeypatch):
    from esr_hip import local

    def refuse(*a, **k):
        raise AssertionError('the CPU path of esr_hip.local ran inside a GPU test')
    monkeypatch.setattr(local, '_patch_std_cpu', refuse)
    monkeypatch.setattr(local, '_shift_l1_cpu', refuse)


def golden():
    return np.load(GOLDEN)


def irregular_mask(H, W, seed):
    m = (seeded_uniform((H, W), seed).numpy() > 0.25).astype(np.float32)
    m[: H // 8] = 0
    m[:, -(W // 9):] = 0
    m[H // 4: 3 * H // 4, W // 6: 2 * W // 3] = 1
    return m


def test_patch_std_matches_float64_at_512x384():
    from esr_hip import local
    H, W = 512, 384
    ps = local.PatchSet(irregular_mask(H, W, 1501), H, W)
    x = seeded_uniform((2, 3, H, W), 1502, -0.1, 1.1).to(DEV)
    x[:, :, 100:140, 50:90] = 0.5                                         # some flat windows (S = 0) inside the region
    x.requires_grad_(True)
    S = local.patch_std(x, ps)
    x64 = x.detach().double().requires_grad_(True)
    S64 = std64(x64, ps)
    assert S.shape == S64.shape == (ps.P, 2)
    s, r = S.detach().double(), S64.detach()
    big = r > 1e-3
    assert big.any() and (~big).any()
    assert float(((s - r).abs() / r)[big].max()) <= 1e-5
    assert float((s - r).abs()[~big].max()) <= 1e-7
    cot = seeded_uniform(tuple(S.shape), 1503, -1.0, 1.0).to(DEV)
    (S * cot).sum().backward()
    (S64 * cot.double()).sum().backward()
    g, g64 = x.grad.double(), x64.grad
    assert torch.isfinite(x.grad).all()
    assert float((g - g64).abs().max()) <= 1e-5 * float(g64.abs().max())


@pytest.mark.parametrize('H,W,P', [(7, 7, 1), (22, 70, 1024), (23, 71, 1105)])
def test_patch_std_matches_float64_at_the_tile_frame_edges(H, W, P):
    """the smallest shapes at which the shared 16 x 64 corner-tile frame can go wrong, full mask: one corner in a tile that is almost all padding;
    Hc x Wc = 16 x 64, exactly one full tile; 17 x 65, a 2 x 2 grid whose last row and column of tiles hold one corner each.  The bounds of
    test_patch_std_matches_float64_at_512x384 (these inputs have no flat windows, so both sides of its split need not occur)."""
    from esr_hip import local
    ps = local.PatchSet(None, H, W)
    assert ps.P == P
    x = seeded_uniform((2, 3, H, W), 1508, -0.1, 1.1).to(DEV).requires_grad_(True)
    S = local.patch_std(x, ps)
    x64 = x.detach().double().requires_grad_(True)
    S64 = std64(x64, ps)
    assert S.shape == S64.shape == (P, 2)
    s, r = S.detach().double(), S64.detach()
    big = r > 1e-3
    print('patch_std %d x %d: P %d, %d of %d STDs above 1e-3, worst rel %.2e' % (H, W, P, int(big.sum()), big.numel(),
                                                                               float(((s - r).abs() / r)[big].max()) if big.any() else 0.0))
    if big.any():
        assert float(((s - r).abs() / r)[big].max()) <= 1e-5
    if (~big).any():
        assert float((s - r).abs()[~big].max()) <= 1e-7
    cot = seeded_uniform(tuple(S.shape), 1509, -1.0, 1.0).to(DEV)
    (S * cot).sum().backward()
    (S64 * cot.double()).sum().backward()
    g, g64 = x.grad.double(), x64.grad
    print('   grad err / max|grad| %.2e' % (float((g - g64).abs().max()) / float(g64.abs().max())))
    assert torch.isfinite(x.grad).all()
    assert float((g - g64).abs().max()) <= 1e-5 * float(g64.abs().max())
    again = x.detach().clone().requires_grad_(True)
    (local.patch_std(again, ps) * cot).sum().backward()
    assert torch.equal(x.grad, again.grad)


def test_flat_patch_gradient_is_zero_and_finite():
    from esr_hip import local
    x = torch.full((1, 3, 16, 16), 0.3, device=DEV)
    x[:, :, :, 12:] = seeded_uniform((1, 3, 16, 4), 1504).to(DEV)
    x.requires_grad_(True)
    S = local.patch_std(x, local.PatchSet(None, 16, 16))
    assert float(S[0, 0]) == 0.0
    S.sum().backward()
    assert torch.isfinite(x.grad).all()
    assert float(x.grad[..., :5].abs().max()) == 0.0                     # columns 0..4: covered by flat windows only (cx <= 4)


def test_patch_std_backward_is_deterministic_and_per_image():
    from esr_hip import local
    H, W = 200, 232
    ps = local.PatchSet(irregular_mask(H, W, 1505), H, W)
    x = seeded_uniform((4, 3, H, W), 1506, -0.1, 1.1).to(DEV)
    cot = seeded_uniform((ps.P, 4), 1507, -1.0, 1.0).to(DEV)

    def grad(xx, c):
        xx = xx.clone().requires_grad_(True)
        (local.patch_std(xx, ps) * c).sum().backward()
        return xx.grad
    g1, g2 = grad(x, cot), grad(x, cot)
    assert torch.equal(g1, g2)
    halves = torch.cat([grad(x[:2], cot[:, :2]), grad(x[2:], cot[:, 2:])])
    assert torch.equal(g1, halves)
    assert torch.equal(local.patch_std(x, ps)[:, 2:], local.patch_std(x[2:], ps))


@pytest.mark.parametrize('interp,points', [(True, [(2.5, 3.25)]), (True, [(2.5, 3.25), (-1.75, 4.5)]), (True, [(-7.3, 0)]), (False, [(3, -2)]),
                                           (False, [(0, 5), (-4, 1)])])
def test_shift_l1_matches_float64_grid_sample(interp, points):
    from esr_hip import local
    H, W = 72, 104
    mask = torch.from_numpy(irregular_mask(H, W, 1508)).to(DEV)
    pairs = [local.ShiftPair(p, H, W, interpolated=interp) for p in points]
    x = seeded_uniform((3, 3, H, W), 1509, -0.1, 1.1).to(DEV).requires_grad_(True)
    loss = local.shift_l1(x, mask, pairs)
    x64 = x.detach().double().requires_grad_(True)
    loss64 = shift64(x64, mask.double(), pairs)
    np.testing.assert_allclose(loss.detach().cpu().numpy(), loss64.detach().cpu().numpy(), rtol=1e-5)
    cot = torch.tensor([1.0, -0.5, 2.0], device=DEV)
    (loss * cot).sum().backward()
    (loss64 * cot.double()).sum().backward()
    g, g64 = x.grad.double(), x64.grad
    assert float((g - g64).abs().max()) <= 1e-5 * float(g64.abs().max())
    g1 = x.grad.clone()
    x.grad = None
    (local.shift_l1(x, mask, pairs) * cot).sum().backward()
    assert torch.equal(g1, x.grad)                                        # no atomics: bit-identical


def test_function_level_values_match_the_reference():
    from esr_hip import local
    g = golden()
    mask = g['a/mask']
    H, W = mask.shape
    ps = local.PatchSet(mask, H, W)
    x = torch.from_numpy(g['a/x']).to(DEV).requires_grad_(True)
    S = local.patch_std(x, ps)
    np.testing.assert_allclose(S.detach().cpu().numpy(), g['a/std/S'], rtol=1e-4, atol=1e-6)
    (S * torch.from_numpy(g['a/std/cot']).to(DEV)).sum().backward()
    gr = g['a/std/grad']
    np.testing.assert_allclose(x.grad.cpu().numpy(), gr, rtol=1e-4, atol=1e-4 * np.abs(gr).max())
    for case in ('nonint1', 'nonint2', 'int1'):
        x = torch.from_numpy(g['a/x']).to(DEV).requires_grad_(True)
        pairs = [local.ShiftPair(p, H, W, interpolated='nonint' in case) for p in g['a/%s/points' % case]]
        initial = local.patch_std(x[:1].detach(), ps)
        loss = (20 * (local.patch_std(x, ps) - initial) ** 2).mean() + local.shift_l1(x, torch.from_numpy(mask).to(DEV), pairs)
        np.testing.assert_allclose(loss.detach().cpu().numpy(), g['a/%s/loss' % case], rtol=1e-4)
        loss.sum().backward()
        gr = g['a/%s/grad' % case]
        np.testing.assert_allclose(x.grad.cpu().numpy(), gr, rtol=1e-4, atol=1e-4 * np.abs(gr).max())


def product_opt():
    """the options gen_F7 gave the reference (oracle/gen_golden.py::_ref_opt, inference)"""
    from options.options import dict_to_nonedict
    return dict_to_nonedict({
        'name': 'f7', 'model': 'srragan', 'scale': 4, 'gpu_ids': [0], 'range': [0, 1], 'is_train': False,
        'path': {'root': RUN_DIR, 'models': os.path.join(RUN_DIR, 'models'), 'log': RUN_DIR, 'val_images': RUN_DIR},
        'network_G': {'which_model_G': 'RRDB_net', 'CEM_arch': 1, 'sigmoid_range_limit': 0, 'latent_input': 'all_layers', 'latent_input_domain': 'HR_downscaled',
                      'latent_channels': 3, 'norm_type': None, 'mode': 'CNA', 'nf': 64, 'nb': 1, 'in_nc': 3, 'out_nc': 3, 'gc': 32, 'group': 1, 'scale': 4},
        'network_D': {'which_model_D': 'discriminator_vgg_128', 'relativistic': 0, 'decomposed_input': 0, 'pre_clipping': 0, 'add_quantization_noise': 0,
                      'norm_type': 'batch', 'act_type': 'leakyrelu', 'mode': 'CNA', 'n_layers': 10, 'nf': 64, 'in_nc': 3},
        'datasets': {'train': {'patch_size': 208, 'batch_size': 2}}, 'train': None, 'test': {'kernel': None}})


@pytest.mark.parametrize('mask_name', ['full', 'irr'])
@pytest.mark.parametrize('objective', ['local_STD_increase', 'local_max_STD', 'local_STD_TV', 'local_STD_nonInt_periodicity'])
def test_z_optimizer_matches_the_reference_run(objective, mask_name):
    import models
    from Z_optimization import Z_optimizer
    g = golden()
    m = models.create_model(product_opt())
    fill_formula_weights(m.netG, gain=0.5)
    lr = seeded_uniform((1, 3, 24, 28), 920).to(m.device)
    B = 3
    z0 = seeded_uniform((B, 3, 96, 112), 921, -0.3, 0.3).to(m.device)
    if mask_name == 'full':
        im_mask = z_mask = np.ones([96, 112], dtype=np.float32)
    else:
        im_mask, z_mask = g['b/mask/irr_image'], g['b/mask/irr_Z']
    m.feed_data({'LR': lr.expand(B, -1, -1, -1).clone(), 'Z': z0.clone()}, need_GT=False)
    m.test()
    data = {'LR': lr.expand(B, -1, -1, -1).clone(), 'STD_increment': 0.01, 'periodicity_points': [[2.5, 3.25], [-1.75, 4.5]]}
    zo = Z_optimizer(objective=objective, Z_size=[96, 112], model=m, Z_range=1, max_iters=4, data=data, initial_Z=z0.clone(), initial_LR=0.1, batch_size=B,
                     image_mask=im_mask, Z_mask=z_mask)
    key = 'b/%s/%s/' % (objective, mask_name)
    # (the reference's desired_STD aliases its initial_STD, Z_optimization.py:463-468: after construction both hold initial + increment)
    std0 = zo.desired_STD if 'increase' in objective else zo.initial_STD
    assert std0.shape == g[key + 'initial_STD'].shape
    np.testing.assert_allclose(std0.cpu().numpy(), g[key + 'initial_STD'], rtol=1e-4, atol=1e-6)
    z = zo.optimize()
    ref_loss = g[key + 'loss']
    assert len(zo.loss_values) == len(ref_loss)
    np.testing.assert_allclose(zo.loss_values, ref_loss, rtol=1e-3, atol=1e-3 * abs(ref_loss[0]))
    d = np.abs(z[:, :, ::8, ::8].cpu().numpy() - g[key + 'final_Z_sub'])
    assert np.median(d) < 1e-3 and np.mean(d > 1e-2) < 0.02, (float(np.median(d)), float(np.mean(d > 1e-2)))
    outside = torch.from_numpy(z_mask == 0).to(z.device)
    if outside.any():
        assert float((z - z0).abs()[:, :, outside].max()) < 1e-6          # outside the Z mask nothing moved

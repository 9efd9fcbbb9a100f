"""GPU tests (-m gpu) of the patch-magnitude and periodicityPlus Z objectives (csrc/esr_patchmag.hip through esr_hip/patchmag.py, the region
constraint on csrc/esr_scribble.hip; reference codes/Z_optimization.py:385-394, 450-455, 470-477, 717-726, 743-746, 799-806):
  * the patch-magnitude kernels against a float64 restatement (value, gradient) at 67 x 93 and 512 x 384, the exact zero of the gradient
    outside the selected windows, determinism, batch independence;
  * the region-constraint helper against F.l1_loss in float64;
  * the reference's own values (tests/golden/special_z.npz, tools/gen_special_z_golden.py): function level (a) and Z_optimizer.optimize()
    runs on the F7 model (b), with and without the region constraint.
The CPU fallbacks of esr_hip.patchmag, esr_hip.local and esr_hip.scribble are patched to raise for every test here: what is graded is the
kernels."""
import atexit
import os
import shutil
import sys
import tempfile

import numpy as np
import pytest
import torch

from oracle.weights import fill_formula_weights, seeded_uniform

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'special_z.npz')
RUN_DIR = tempfile.mkdtemp(prefix='esr_special_z_')
atexit.register(shutil.rmtree, RUN_DIR, True)
DEV = 'cuda'
INCREMENT = 0.03
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:          # the host test module's fixtures helpers (mag_spec, plus_loss)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def kernels_only(monkeypatch):
    from esr_hip import local, patchmag, scribble

    def refuse(*a, **k):
        raise AssertionError('a CPU path of the Z objectives ran inside a GPU test')
    monkeypatch.setattr(patchmag, '_patch_mag_cpu', refuse)
    monkeypatch.setattr(local, '_patch_std_cpu', refuse)
    monkeypatch.setattr(local, '_shift_l1_cpu', refuse)
    monkeypatch.setattr(scribble, '_scribble_cpu', refuse)


def golden():
    return np.load(GOLDEN)


def irregular_mask(H, W, seed):
    m = (seeded_uniform((H, W), seed).numpy() > 0.25).astype(np.float32)
    m[: H // 8] = 0
    m[:, -(W // 9):] = 0
    m[H // 4: 3 * H // 4, W // 6: 2 * W // 3] = 1
    return m


def mag64(x, spec):
    """float64 restatement: per image the mean over the 49 x P entries of (patches(mean_c clamp(x, 0, 1)) - desired)^2 -> [B]"""
    v = torch.clamp(x, 0, 1).mean(1).reshape(x.size(0), -1)
    idx = torch.from_numpy(spec.patches).to(x.device)
    return ((v[:, idx] - spec.desired.t().to(x.device).double()) ** 2).mean(dim=(1, 2))


def make_spec(H, W, mask, seed, sign=1):
    from esr_hip import patchmag
    I0 = torch.clamp(seeded_uniform((3, H, W), seed, -0.1, 1.1), 0, 1)
    I0[:, H // 3: H // 3 + 12, W // 4: W // 4 + 12] = 0.5                 # flat patches: the 1/255 floor
    return patchmag.MagSpec(mask, H, W, I0, INCREMENT, sign)


# the smallest shapes at which the 16 x 64 corner-tile frame shared with the patch-STD kernels can go wrong (full mask, batch 2), with their patch
# counts: one corner in a tile that is almost all padding; Hc x Wc = 16 x 64, exactly one full tile; 17 x 65, a 2 x 2 grid whose last row and
# column of tiles hold one corner each
FRAME_EDGE_P = {(7, 7): 1, (22, 70): 47, (23, 71): 57}


@pytest.mark.parametrize('H,W,masked', [(67, 93, True), (67, 93, False), (512, 384, True), (512, 384, False)] + [s + (False,) for s in FRAME_EDGE_P])
def test_patch_mag_matches_float64(H, W, masked):
    from esr_hip import patchmag
    spec = make_spec(H, W, irregular_mask(H, W, 1801) if masked else None, 1802, -1 if masked else 1)
    B = 2 if (H, W) in FRAME_EDGE_P else 3
    x = seeded_uniform((B, 3, H, W), 1803, -0.1, 1.1).to(DEV).requires_grad_(True)
    loss = patchmag.patch_mag(x, spec)
    x64 = x.detach().double().requires_grad_(True)
    loss64 = mag64(x64, spec)
    assert loss.shape == (B,) and (spec.P == FRAME_EDGE_P[(H, W)] if (H, W) in FRAME_EDGE_P else spec.P > 20)
    rel = float(((loss.detach().double() - loss64.detach()).abs() / loss64.detach()).max())
    cot = torch.tensor([1.0, -0.5, 2.0], device=DEV)[:B]
    (loss * cot).sum().backward()
    (loss64 * cot.double()).sum().backward()
    g, g64 = x.grad.double(), x64.grad
    err = float((g - g64).abs().max()) / float(g64.abs().max())
    print('patch_mag %d x %d masked=%s: P %d, loss rel %.2e, grad err / max|grad| %.2e' % (H, W, masked, spec.P, rel, err))
    assert rel <= 1e-5
    assert torch.isfinite(x.grad).all()
    assert err <= 1e-5


def test_unselected_region_gets_exactly_zero_gradient():
    from esr_hip import patchmag
    H, W = 67, 93
    mask = np.zeros((H, W), np.float32)
    mask[10:40, 20:60] = 1
    spec = make_spec(H, W, mask, 1804)
    x = seeded_uniform((2, 3, H, W), 1805, -0.1, 1.1).to(DEV).requires_grad_(True)
    patchmag.patch_mag(x, spec).sum().backward()
    covered = np.zeros(H * W, bool)
    covered[spec.patches.reshape(-1)] = True
    covered = torch.from_numpy(covered.reshape(H, W)).to(DEV)
    assert covered.any() and not covered[:10].any() and not covered[:, 60:].any()
    assert float(x.grad[:, :, ~covered].abs().max()) == 0.0
    inside = (x.detach() > 0) & (x.detach() < 1) & covered
    assert float((x.grad[inside] != 0).float().mean()) > 0.99             # and the covered pixels inside the clamp's range do get one
    assert float(x.grad[(x.detach() < 0) | (x.detach() > 1)].abs().max()) == 0.0


def test_patch_mag_is_bitwise_deterministic_and_per_image():
    from esr_hip import patchmag
    H, W = 200, 232
    spec = make_spec(H, W, irregular_mask(H, W, 1806), 1807)
    x = seeded_uniform((4, 3, H, W), 1808, -0.1, 1.1).to(DEV)
    cot = torch.tensor([1.0, -0.5, 2.0, 0.25], device=DEV)

    def run(xx, c):
        xx = xx.clone().requires_grad_(True)
        loss = patchmag.patch_mag(xx, spec)
        (loss * c).sum().backward()
        return loss.detach(), xx.grad
    (l1, g1), (l2, g2) = run(x, cot), run(x, cot)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    la, ga = run(x[:2], cot[:2])
    lb, gb = run(x[2:], cot[2:])
    assert torch.equal(l1, torch.cat([la, lb])) and torch.equal(g1, torch.cat([ga, gb]))
    # changing the other images changes nothing of image 1
    y = x.clone()
    y[0], y[2], y[3] = y[0] * 0.5, 1 - y[2], y[3] + 0.1
    l3, g3 = run(y, cot)
    assert torch.equal(l3[1], l1[1]) and torch.equal(g3[1], g1[1])


def test_region_constraint_matches_float64_l1_loss():
    import torch.nn.functional as F
    from esr_hip import scribble
    H, W, B = 67, 93, 3
    mask = irregular_mask(H, W, 1809)
    cm = torch.from_numpy((mask <= 0).astype(np.float64)).to(DEV)
    x = seeded_uniform((B, 3, H, W), 1810, -0.1, 1.1).to(DEV).requires_grad_(True)
    for nb in (B, 1):
        initial = seeded_uniform((nb, 3, H, W), 1811).to(DEV)
        got = scribble.region_constraint(x, mask, initial)
        x64 = x.detach().double().requires_grad_(True)
        want = F.l1_loss(torch.clamp(x64, 0, 1) * cm, (initial.double() * cm).expand(B, -1, -1, -1))
        np.testing.assert_allclose(float(got.detach()), float(want.detach()), rtol=1e-5)
        g, = torch.autograd.grad(got, x)
        g64, = torch.autograd.grad(want, x64)
        assert float((g.double() - g64).abs().max()) <= 1e-5 * float(g64.abs().max())


def test_function_level_values_match_the_reference():
    from esr_hip import patchmag
    from test_host_special_z import mag_spec, plus_loss
    g = golden()
    for sign in ('increase', 'decrease'):
        spec = mag_spec(g, sign)
        x = torch.from_numpy(g['a/x']).to(DEV).requires_grad_(True)
        loss = patchmag.patch_mag(x, spec)
        np.testing.assert_allclose(loss.detach().cpu().numpy(), g['a/mag/%s/loss' % sign], rtol=1e-4)
        loss.sum().backward()
        gr = g['a/mag/%s/grad' % sign]
        np.testing.assert_allclose(x.grad.cpu().numpy(), gr, rtol=1e-4, atol=1e-4 * np.abs(gr).max())
    for case in ('nonint1', 'nonint2', 'whole'):
        x = torch.from_numpy(g['a/x']).to(DEV).requires_grad_(True)
        loss, desired = plus_loss(g, case, x, DEV)
        np.testing.assert_allclose(desired.cpu().numpy(), g['a/plus/%s/desired_STD' % case], rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(loss.detach().cpu().numpy(), g['a/plus/%s/loss' % case], rtol=1e-4)
        loss.sum().backward()
        gr = g['a/plus/%s/grad' % case]
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


@pytest.mark.parametrize('case', ['full', 'irr', 'irr_nonlocal'])
@pytest.mark.parametrize('objective', ['local_Mag_increase', 'local_STD_nonInt_periodicityPlus'])
def test_z_optimizer_matches_the_reference_run(objective, case):
    """Figures of this test: DESIGN.md section 3.12."""
    import models
    from Z_optimization import Z_optimizer
    g = golden()
    m = models.create_model(product_opt())
    fill_formula_weights(m.netG, gain=0.5)
    lr = seeded_uniform((1, 3, 24, 28), 920).to(m.device)
    B = 3
    non_local = case == 'irr_nonlocal'
    z0 = seeded_uniform((B, 3, 96, 112), 921, -0.3, 0.3).to(m.device)          # the model's current output ...
    z1 = seeded_uniform((B, 3, 96, 112), 922, -0.3, 0.3).to(m.device)          # ... and, with the constraint, the search's start (no ties in it)
    start = z1 if non_local else z0
    if case == 'full':
        im_mask = z_mask = np.ones([96, 112], dtype=np.float32)
    else:
        im_mask, z_mask = g['b/mask/irr_image'], g['b/mask/irr_Z']
    n0 = 1 if 'Mag' in objective else B               # the reference builds its desired patches from a batch of one
    m.feed_data({'LR': lr.expand(n0, -1, -1, -1).clone(), 'Z': z0[:n0].clone()}, need_GT=False)
    m.test()
    data = {'LR': lr.expand(B, -1, -1, -1).clone(), 'STD_increment': INCREMENT, 'periodicity_points': [[2.5, 3.25], [-1.75, 4.5]]}
    zo = Z_optimizer(objective=objective, Z_size=[96, 112], model=m, Z_range=1, max_iters=4, data=data, initial_Z=start.clone(), initial_LR=0.1,
                     batch_size=B, image_mask=im_mask, Z_mask=z_mask, non_local_Z_optimization=non_local)
    key = 'b/%s/%s/' % (objective, case)
    assert zo.non_local_Z_optimization == non_local
    np.testing.assert_array_equal(np.asarray(zo.Z_mask, dtype=np.float32), g[key + 'Z_mask'])
    z = zo.optimize()
    ref_loss = g[key + 'loss']
    d = np.abs(z[:, :, ::8, ::8].cpu().numpy() - g[key + 'final_Z_sub'])
    print('%s %s: loss rel %.2e, median |dZ| %.2e, fraction of |dZ| > 1e-2 %.4f' % (
        objective, case, float(np.max(np.abs(np.array(zo.loss_values) - ref_loss[:len(zo.loss_values)]) / np.abs(ref_loss[:len(zo.loss_values)]))),
        float(np.median(d)), float(np.mean(d > 1e-2))))
    assert len(zo.loss_values) == len(ref_loss)
    np.testing.assert_allclose(zo.loss_values, ref_loss, rtol=1e-3)
    assert np.median(d) < 1e-3 and np.mean(d > 1e-2) <= 0.02, (float(np.median(d)), float(np.mean(d > 1e-2)))
    outside = torch.from_numpy(g[key + 'Z_mask'] == 0).to(z.device)
    if case != 'full':
        assert outside.any()
        assert float((z - start).abs()[:, :, outside].max()) < 1e-6           # outside the (rebuilt) Z mask nothing moved

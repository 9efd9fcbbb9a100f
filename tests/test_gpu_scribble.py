"""GPU tests (-m gpu) of the scribble Z objective and its region constraint (csrc/esr_scribble.hip through esr_hip/scribble.py; reference
codes/Z_optimization.py:344-364, 385-390, 401-448, 743-746):
  * the kernels against a float64 torch restatement (value, gradient) with every label kind, border-touching regions, I0 of batch 1 and B,
    and one larger size; empty terms give exactly 0; determinism and batch independence;
  * the reference's own values (tests/golden/scribble.npz, tools/gen_scribble_golden.py): function level (a) and Z_optimizer.optimize() runs
    on the F7 model with the region constraint off and on (b).
The CPU fallback of esr_hip.scribble is patched to raise for every test here: what is graded is the kernels."""
import atexit
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch

from oracle.weights import fill_formula_weights, seeded_uniform

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'scribble.npz')
RUN_DIR = tempfile.mkdtemp(prefix='esr_scribble_')
atexit.register(shutil.rmtree, RUN_DIR, True)
DEV = 'cuda'


@pytest.fixture(autouse=True)
def kernels_only(monkeypatch):
    from esr_hip import scribble

    def refuse(*a, **k):
        raise AssertionError('the CPU path of esr_hip.scribble ran inside a GPU test')
    monkeypatch.setattr(scribble, '_scribble_cpu', refuse)


def golden():
    return np.load(GOLDEN)


def case(H, W, seed):
    """an irregular image mask and a label map with every kind: colour, brighten, darken, TV regions touching the border and each other"""
    g = torch.Generator().manual_seed(seed)
    mask = (torch.rand(H, W, generator=g) > 0.2).numpy().astype(np.float32)
    mask[: H // 6] = 0
    mask[H // 3: 2 * H // 3, W // 5: 4 * W // 5] = 1
    s = np.zeros((H, W), np.int64)
    s[H // 5: H // 2, : W // 4] = 1
    s[H // 2:, : W // 6] = 2
    s[H // 2:, W // 6: W // 3] = 3
    s[H // 4:, W // 3: W // 2] = 4                          # touches the bottom border and region 5
    s[H // 4:, W // 2: 2 * W // 3] = 5
    s[: H // 3, 2 * W // 3:] = 11                           # touches the top and right borders (partly outside the mask)
    s[2 * H // 3:, 5 * W // 6:] = 50
    s[H // 2: H // 2 + 3, 2 * W // 3 + 2: 2 * W // 3 + 5] = 1
    return mask, s


def loss64(x, mask, s, D, I0, norm):
    """float64 restatement: (L [B], C) with one mask per TV region, as the reference loops over them"""
    x, D = x.double(), D.double()
    I = torch.clamp(x, 0, 1)
    lm = torch.from_numpy(mask > 0).to(x.device)
    st = torch.from_numpy(s).to(x.device)
    M1 = (lm & (st > 0) & (st < 4)).double()
    L = (M1 * (I - D).abs()).mean(dim=(1, 2, 3))
    H, W = mask.shape
    for k in [k for k in torch.unique(st * lm).tolist() if k > 3]:
        R = (lm & (st == k)).double()
        for dy, dx in ((1, 1), (1, 0), (0, 1), (-1, 1)):
            y0, y1, x0, x1 = max(-dy, 0), H - max(dy, 0), max(-dx, 0), W - max(dx, 0)
            m = R[y0:y1, x0:x1] * R[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
            L = L + (m * (I[:, :, y0:y1, x0:x1] - I[:, :, y0 + dy:y1 + dy, x0 + dx:x1 + dx]).abs()).mean(dim=(1, 2, 3))
    if I0 is None:
        return L, torch.zeros((), dtype=torch.float64, device=x.device)
    return L, ((~lm).double() * (I - I0.double()).abs()).sum() / norm


def run(x, spec, gL, gC, norm=None):
    from esr_hip import scribble
    x = x.clone().requires_grad_(True)
    L, C = scribble.scribble_loss(x, spec, norm)
    ((L * gL).sum() + gC * C).backward()
    return L.detach(), C.detach(), x.grad


@pytest.mark.parametrize('H,W,B,i0_batch', [(67, 93, 3, 1), (67, 93, 3, 3), (512, 384, 2, 2)])
def test_kernels_match_float64(H, W, B, i0_batch):
    from esr_hip import scribble
    mask, s = case(H, W, H + W)
    x = seeded_uniform((B, 3, H, W), 1600 + H, -0.1, 1.1).to(DEV)
    D = seeded_uniform((1, 3, H, W), 1601, -0.05, 1.2).to(DEV)
    I0 = seeded_uniform((i0_batch, 3, H, W), 1602, 0, 1).to(DEV)
    x[0, :, 5, 5] = 1.0                                        # clamp bounds are inside (torch passes the gradient at 0 and 1)
    x[0, :, 6, 6] = 0.0
    spec = scribble.ScribbleSpec(s, mask, D, constraint=True, initial=I0)
    gL = torch.tensor([1.0, -0.5, 2.0][:B], device=DEV)
    L, C, dx = run(x, spec, gL, 0.7)
    x64 = x.double().clone().requires_grad_(True)
    L64, C64 = loss64(x64, mask, s, D, I0, B * 3 * H * W)
    ((L64 * gL.double()).sum() + 0.7 * C64).backward()
    np.testing.assert_allclose(L.cpu().numpy(), L64.detach().cpu().numpy(), rtol=1e-5)
    np.testing.assert_allclose(float(C), float(C64.detach()), rtol=1e-5)
    g64 = x64.grad.cpu().numpy()
    np.testing.assert_allclose(dx.cpu().numpy(), g64, rtol=1e-5, atol=1e-5 * np.abs(g64).max())


def test_empty_terms_give_exactly_zero():
    from esr_hip import scribble
    H, W, B = 40, 56, 2
    x = seeded_uniform((B, 3, H, W), 1610, -0.1, 1.1).to(DEV)
    D = seeded_uniform((1, 3, H, W), 1611).to(DEV)
    full = np.ones((H, W), np.float32)
    only_tv = np.zeros((H, W), np.int64)
    only_tv[5:30, 5:40] = 4
    only_l1 = np.zeros((H, W), np.int64)
    only_l1[5:30, 5:40] = 1
    for s, constraint in ((only_tv, False), (only_l1, False), (np.zeros((H, W), np.int64), False), (only_l1, True)):
        spec = scribble.ScribbleSpec(s, full, D, constraint=constraint, initial=torch.clamp(x, 0, 1)[:1] if constraint else None)
        L, C, dx = run(x, spec, torch.ones(B, device=DEV), 1.0)
        assert float(C) == 0.0                                   # off, or a full mask: nothing outside it
        if not s.any():
            assert float(L.abs().max()) == 0.0 and float(dx.abs().max()) == 0.0
    # the L1 term alone: the TV sums are exactly 0, so L is the L1 mean alone
    spec = scribble.ScribbleSpec(only_l1, full, D)
    L, _, _ = run(x, spec, torch.ones(B, device=DEV), 0.0)
    l1 = ((torch.from_numpy(only_l1 == 1).to(DEV).double() * (torch.clamp(x, 0, 1).double() - D.double()).abs()).mean(dim=(1, 2, 3)))
    np.testing.assert_allclose(L.cpu().numpy(), l1.cpu().numpy(), rtol=1e-6)


def test_bitwise_deterministic_and_independent_per_image():
    from esr_hip import scribble
    H, W, B = 67, 93, 3
    mask, s = case(H, W, 7)
    x = seeded_uniform((B, 3, H, W), 1620, -0.1, 1.1).to(DEV)
    D = seeded_uniform((1, 3, H, W), 1621).to(DEV)
    I0 = seeded_uniform((B, 3, H, W), 1622).to(DEV)
    spec = scribble.ScribbleSpec(s, mask, D, constraint=True, initial=I0)
    gL = torch.tensor([1.0, 2.0, 3.0], device=DEV)
    a, b = run(x, spec, gL, 0.5), run(x, spec, gL, 0.5)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    # image 1 alone (its own I0) gives the same loss and gradient as inside the batch
    spec1 = scribble.ScribbleSpec(s, mask, D, constraint=True, initial=I0[1:2])
    L1, _, dx1 = run(x[1:2], spec1, gL[1:2], 0.5, norm=B * 3 * H * W)
    np.testing.assert_allclose(float(L1[0]), float(a[0][1]), rtol=1e-6)         # (the row sums reduce in a batch-shaped torch sum)
    assert torch.equal(dx1[0], a[2][1])


def test_function_level_values_match_the_reference():
    from esr_hip import scribble
    g = golden()
    I0 = torch.clamp(torch.from_numpy(g['a/x_init']), 0, 1).to(DEV)
    D = scribble.desired_image(g['a/desired_in'], g['a/scribble'], I0[0], 0.3)
    np.testing.assert_allclose(D, g['a/D'], rtol=1e-5, atol=1e-6)
    spec = scribble.ScribbleSpec(g['a/scribble'], g['a/mask'], D, constraint=True, initial=I0)
    x = torch.from_numpy(g['a/x']).to(DEV)
    L, C, dx = run(x, spec, torch.ones(x.size(0), device=DEV), 0.0)
    np.testing.assert_allclose(L.cpu().numpy(), g['a/loss'], rtol=1e-4)
    np.testing.assert_allclose(float(C), float(g['a/constraint']), rtol=1e-4)
    gr = g['a/grad_loss']
    np.testing.assert_allclose(dx.cpu().numpy(), gr, rtol=1e-4, atol=1e-4 * np.abs(gr).max())
    _, _, dx = run(x, spec, torch.zeros(x.size(0), device=DEV), 1.0)
    gr = g['a/grad_constraint']
    np.testing.assert_allclose(dx.cpu().numpy(), gr, rtol=1e-4, atol=1e-4 * np.abs(gr).max())


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


@pytest.mark.parametrize('mode', ['local', 'nonlocal'])
def test_z_optimizer_matches_the_reference_run(mode):
    import models
    from Z_optimization import Z_optimizer
    g = golden()
    m = models.create_model(product_opt())
    fill_formula_weights(m.netG, gain=0.5)
    lr = seeded_uniform((1, 3, 24, 28), 920).to(m.device)
    B = 3
    z0 = seeded_uniform((B, 3, 96, 112), 921, -0.3, 0.3).to(m.device)          # the model's current output ...
    z1 = seeded_uniform((B, 3, 96, 112), 922, -0.3, 0.3).to(m.device)          # ... and the search's start (no ties in the constraint)
    m.feed_data({'LR': lr.expand(B, -1, -1, -1).clone(), 'Z': z0.clone()}, need_GT=False)
    m.test()
    data = {'LR': lr.expand(B, -1, -1, -1).clone(), 'desired': torch.from_numpy(g['b/desired_in']).to(m.device), 'scribble_mask': g['b/scribble'],
            'brightness_factor': 0.3}
    zo = Z_optimizer(objective='scribble', Z_size=[96, 112], model=m, Z_range=1, max_iters=4, data=data, initial_Z=z1.clone(), initial_LR=0.1,
                     batch_size=B, image_mask=g['b/mask/image'], Z_mask=g['b/mask/Z'], non_local_Z_optimization=mode == 'nonlocal')
    key = 'b/%s/' % mode
    np.testing.assert_array_equal(np.asarray(zo.Z_mask, dtype=np.float32), g[key + 'Z_mask'])
    z = zo.optimize()
    ref_loss = g[key + 'loss']
    assert len(zo.loss_values) == len(ref_loss)
    np.testing.assert_allclose(zo.loss_values, ref_loss, rtol=1e-3, atol=1e-3 * abs(ref_loss[0]))
    d = np.abs(z[:, :, ::8, ::8].cpu().numpy() - g[key + 'final_Z_sub'])
    assert np.median(d) < 1e-3 and np.mean(d > 1e-2) < 0.02, (float(np.median(d)), float(np.mean(d > 1e-2)))
    outside = torch.from_numpy(g[key + 'Z_mask'] == 0).to(z.device)
    assert outside.any()
    assert float((z - z1).abs()[:, :, outside].max()) < 1e-6          # outside the (rebuilt) Z mask nothing moved

"""GPU tests (-m gpu) of the random-alternatives Z objectives (csrc/esr_pairmin.hip through esr_hip/pairmin.py and Z_optimization.py; reference
codes/Z_optimization.py:365, :546-550, :683-701, :765-766):
  * the kernels against a float64 evaluation of the definition on the same inputs (values, gradients; masks, the limited term, sub-ranges of
    the batch, saturated inputs, W not a multiple of 64, B up to 64 and one batch too large for LDS), determinism, and that nothing of size
    B x B is allocated;
  * the reference's own values (tests/golden/random_z.npz, tools/gen_random_z_golden.py): function level (a) and optimize() runs on the F7
    model (b); 'random_VGG' on the F7-sized model against the CPU fallback on the same features.
The CPU fallback of esr_hip.pairmin is patched to raise where the kernels are graded.

Gradients and ties.  The loss is a min over the other samples; where two of them are equally near, the gradient depends on which one is taken
(the kernel: the lowest index; torch.min: unspecified).  A position (c, h, w) is excluded from the gradient comparison when, in float64, some
row's two smallest distances (the diagonal's 1 included) differ by less than 1e-6 and the two tied neighbours are not both clamped (pre-clamp
value outside (0, 1)): two clamped neighbours sit on the same bound, give the same sign to the row and receive nothing themselves.  The share
of excluded positions is recomputed and asserted to be at most 1 % in every case (measured on an MI355X with this file's seeds: 0.48 - 0.61 % on
uniform [-0.1, 1.1] data at 64 x 3 x 40 x 52, at most 0.02 % at B <= 5, 0.19 - 0.21 % on the unclamped Gaussian cases of B = 64 and 330)."""
import os

import numpy as np
import pytest
import torch

from oracle.weights import fill_formula_weights, seeded_uniform
from oracle.zobj_contract_ref import TIE, definition64

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'random_z.npz')
DEV = 'cuda'


@pytest.fixture
def kernels_only(monkeypatch):
    from esr_hip import pairmin

    def refuse(*a, **k):
        raise AssertionError('the CPU path of esr_hip.pairmin ran inside a GPU test')
    monkeypatch.setattr(pairmin, '_share_cpu', refuse)


def make_case(B, H, W, seed, clamp01, masked, limited, init_batch=None):
    if clamp01:
        x = seeded_uniform((B, 3, H, W), seed, -0.1, 1.1)
        # saturated inputs: the bounds themselves (torch passes the gradient there), every other sample strictly inside at these two pixels
        x[:, :, 5, 5] = 0.3 + 0.4 * seeded_uniform((B, 3), seed + 1)
        x[:, :, 6, 6] = 0.3 + 0.4 * seeded_uniform((B, 3), seed + 2)
        x[0, :, 5, 5] = 1.0
        x[B - 1, :, 6, 6] = 0.0
    else:
        # feature-like: distances beyond the cap of 1.  (Spread out for the large batch: B^2 near-ties per unit of range would exceed the 1 % rule)
        x = (1.5 if B <= 64 else 20.0) * torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(seed))
    mask = (seeded_uniform((H, W), seed + 3) > 0.3).float() if masked else None
    init = seeded_uniform((init_batch or B, 3, H, W), seed + 4, -0.1, 1.1) if limited else None
    dev = lambda t: None if t is None else t.to(DEV)
    return dev(x), dev(mask), dev(init)


def run(x, x_all, lo, clamp01, mask, init, w, g=1.0):
    from esr_hip import pairmin
    x = x.clone().requires_grad_(True)
    Z, share = pairmin.random_share(x, x_all, lo, clamp01=clamp01, mask=mask, init=init, w=w)
    (g * share).backward()
    return Z, share.detach(), x.grad


CASES = [  # B, H, W, clamp01, masked, limited
    (1, 40, 52, True, False, False), (1, 40, 52, True, True, True),
    (2, 33, 70, True, False, True), (2, 33, 70, True, True, False),
    (3, 67, 93, True, True, True), (3, 67, 93, True, False, False), (3, 67, 93, False, False, False),
    (5, 40, 52, True, True, False), (5, 40, 52, True, False, True),
    (64, 40, 52, True, False, False), (64, 40, 52, True, True, True), (64, 19, 37, False, False, False),
    (330, 8, 20, False, True, True),               # beyond what LDS holds: the columns live in global memory
]


@pytest.mark.parametrize('B,H,W,clamp01,masked,limited', CASES)
def test_kernels_match_float64(kernels_only, B, H, W, clamp01, masked, limited):
    w = 0.4
    x, mask, init = make_case(B, H, W, 1900 + B + H, clamp01, masked, limited)
    Z, share, dx = run(x, None, 0, clamp01, mask, init, w, g=0.7)
    x64 = x.double().requires_grad_(True)
    Z64, excluded = definition64(x64, clamp01, mask, init, w)
    (0.7 * Z64.mean()).backward()
    g64 = x64.grad
    frac = float(excluded.float().mean())
    print('B %d %dx%d clamp %d mask %d limited %d: excluded positions %.4f %%, Z rel err %.2e, grad max err / max %.2e' % (
        B, H, W, clamp01, masked, limited, 100 * frac, float(((Z.double() - Z64.detach()).abs() / Z64.detach().abs()).max()),
        float(((dx.double() - g64).abs() * ~excluded).max() / g64.abs().max().clamp_min(1e-300))))
    assert frac <= 0.01
    np.testing.assert_allclose(Z.cpu().numpy(), Z64.detach().cpu().numpy(), rtol=1e-5)
    np.testing.assert_allclose(float(share), float(Z64.detach().mean()), rtol=1e-5)
    keep = (~excluded).expand_as(g64).cpu().numpy()
    g64 = g64.cpu().numpy()
    np.testing.assert_allclose(dx.cpu().numpy()[keep], g64[keep], rtol=1e-5, atol=1e-5 * np.abs(g64).max())
    if B > 1:
        assert np.abs(g64).max() > 0
    # proper sub-ranges [lo, hi): this rank's rows attached, all rows as the detached global batch.  Values and gradients are those of the
    # matching rows of the whole-batch call (the same arithmetic: to the bit), and the shares add up
    if B >= 3:
        total = 0.0
        for lo, hi in ((0, 1), (1, B - 1), (B - 1, B)) if B > 3 else ((0, 2), (2, 3)):
            sub_init = None if init is None else init[lo:hi]
            Zs, shs, dxs = run(x[lo:hi], x, lo, clamp01, mask, sub_init, w, g=0.7)
            assert torch.equal(Zs, Z[lo:hi]) and torch.equal(dxs, dx[lo:hi]), (lo, hi)
            total += float(shs)
        np.testing.assert_allclose(total, float(share), rtol=1e-6)


def test_excluded_share_on_uniform_data():
    """the exclusion rule, measured on this file's own seeds: at most 1 % of positions, at B = 64 and at small B"""
    for B, seed in ((64, 0), (64, 1), (5, 0), (3, 1)):
        x, _, _ = make_case(B, 40, 52, 1990 + seed, True, False, False)
        _, excluded = definition64(x.double(), True, None, None, 0.0)
        frac = float(excluded.float().mean())
        print('B %d seed %d: excluded %.4f %%' % (B, seed, 100 * frac))
        assert frac <= 0.01


def test_broadcast_initial_image_and_lowest_index_on_exact_ties(kernels_only):
    # init of batch 1 broadcasts over the rows
    x, mask, init = make_case(3, 33, 70, 1950, True, True, True, init_batch=1)
    Z, _, dx = run(x, None, 0, True, mask, init, 0.4)
    Zb, _, dxb = run(x, None, 0, True, mask, init.expand(3, -1, -1, -1).contiguous(), 0.4)
    assert torch.equal(Z, Zb) and torch.equal(dx, dxb)
    # an exact tie goes to the lowest index (stated in the kernel's header): rows 1 and 2 are equally far from row 0 on either side of it
    x = torch.tensor([0.5, 0.25, 0.75, 0.0625], device=DEV).view(4, 1, 1, 1).repeat(1, 3, 2, 2).contiguous()
    Z, _, dx = run(x, None, 0, True, None, None, 0.0)
    n = 4 * 3 * 2 * 2                                              # B C H W
    # row 0 -> 1 (tie with 2: lowest index), 1 -> 3 (0.1875 < 0.25), 2 -> 0, 3 -> 1; d loss = -(1 / n) d sum(near)
    want = -torch.tensor([+1 - 1, -1 + 1 + 1, +1, -1 - 1], dtype=torch.float32, device=DEV) / n
    # row 0: own sign(0.5 - 0.25) = +1, received from row 2: sign(0.5 - 0.75) = -1
    # row 1: received from row 0: sign(0.25 - 0.5) = -1; own sign(0.25 - 0.0625) = +1; received from row 3: sign(0.25 - 0.0625) = +1
    # row 2: own sign(0.75 - 0.5) = +1;  row 3: own sign(0.0625 - 0.25) = -1, received from row 1: sign(0.0625 - 0.25) = -1
    assert torch.equal(dx, want.view(4, 1, 1, 1).expand_as(dx))
    np.testing.assert_allclose(Z.cpu().numpy(), -np.array([0.25, 0.1875, 0.25, 0.1875]), rtol=1e-6)


def test_two_calls_are_bit_identical(kernels_only):
    x, mask, init = make_case(64, 67, 93, 1960, True, True, True)
    a, b = run(x, None, 0, True, mask, init, 0.4), run(x, None, 0, True, mask, init, 0.4)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    a, b = run(x[8:24], x, 8, True, mask, init[8:24], 0.4), run(x[8:24], x, 8, True, mask, init[8:24], 0.4)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_nothing_of_size_b_by_b_is_allocated(kernels_only):
    """16 x 3 x 256^2: one [B, B, C, H, W] intermediate is 16 times the bytes of x; forward + backward of the term stay below 4 times"""
    from esr_hip import pairmin
    x = torch.rand(16, 3, 256, 256, generator=torch.Generator().manual_seed(1970)).to(DEV).requires_grad_(True)
    mask = torch.ones(256, 256, device=DEV)
    init = torch.rand(16, 3, 256, 256, generator=torch.Generator().manual_seed(1971)).to(DEV)
    Z, share = pairmin.random_share(x, mask=mask, init=init, w=0.3)         # (library and allocator warm-up)
    share.backward()
    x.grad = None
    del Z, share
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    Z, share = pairmin.random_share(x, mask=mask, init=init, w=0.3)
    share.backward()
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    print('peak growth %.1f MB, x %.1f MB' % (growth / 2 ** 20, x.numel() * 4 / 2 ** 20))
    assert growth < 4 * x.numel() * 4
    assert x.grad is not None and float(x.grad.abs().max()) > 0


def test_function_level_values_match_the_reference(kernels_only):
    from test_host_random_z import fixture_cases, run_fixture_case
    g = np.load(GOLDEN)
    cases = fixture_cases(g)
    assert len(cases) == 13
    for key in cases:
        Z, share, dx = run_fixture_case(g, key, DEV)
        np.testing.assert_allclose(Z, g[key + '/Z_loss'], rtol=1e-4, err_msg=key)
        np.testing.assert_allclose(share, float(g[key + '/loss']), rtol=1e-4, err_msg=key)
        gr = g[key + '/grad']
        np.testing.assert_allclose(dx, gr, rtol=1e-4, atol=1e-4 * max(np.abs(gr).max(), 1e-30), err_msg=key)


@pytest.mark.parametrize('name', ['l1_masks', 'limited'])
def test_z_optimizer_matches_the_reference_run(kernels_only, monkeypatch, name):
    import models
    from test_gpu_scribble import product_opt
    from Z_optimization import Z_optimizer
    g = np.load(GOLDEN)
    m = models.create_model(product_opt())
    fill_formula_weights(m.netG, gain=0.5)
    lr = seeded_uniform((1, 3, 24, 28), 920).to(m.device)
    B = 3
    z0 = seeded_uniform((B, 3, 96, 112), 921, -0.3, 0.3).to(m.device)          # the model's current output ...
    z1 = seeded_uniform((B, 3, 96, 112), 940, -0.3, 0.3).to(m.device)          # ... and the search's start
    m.feed_data({'LR': lr.expand(B, -1, -1, -1).clone(), 'Z': z0.clone()}, need_GT=False)
    m.test()
    data = {'LR': lr.expand(B, -1, -1, -1).clone(), 'rmse_weight': 0.3}
    kw = dict(image_mask=g['b/mask/image'], Z_mask=g['b/mask/Z']) if name == 'l1_masks' else {}
    with monkeypatch.context() as mp:
        mp.setattr(torch, 'randn_like', lambda t, **k: torch.zeros_like(t))     # the fixture pins the 'limited' perturbation of the start to zero
        zo = Z_optimizer(objective='random_l1' if name == 'l1_masks' else 'random_l1_limited', Z_size=[96, 112], model=m, Z_range=1, max_iters=4,
                         data=data, initial_Z=z1.clone(), initial_LR=0.1, batch_size=B, random_Z_inits=False, **kw)
    z = zo.optimize()
    key = 'b/%s/' % name
    ref_loss, ref_last = g[key + 'loss'], g[key + 'Z_loss']
    print(name, 'loss', zo.loss_values, 'reference', ref_loss.tolist(), 'last', zo.latest_Z_loss_values, 'reference', ref_last.tolist())
    assert len(zo.loss_values) == len(ref_loss)
    np.testing.assert_allclose(zo.loss_values, ref_loss, rtol=1e-3, atol=1e-3 * abs(ref_loss[0]))
    assert int(np.argmin(zo.latest_Z_loss_values)) == int(np.argmin(ref_last))
    if name == 'limited':
        assert zo.loss_values[0] == zo.loss_values[1]
    # The final Z: Adam moves an entry by about lr = 0.1 per step along the SIGN of its gradient, so entries whose gradient is at rounding level
    # end elsewhere in any two runs that differ at rounding level.  The fixture records how many do in the reference itself when its input moves
    # by 2e-5 relative, the documented distance of this generator from the fp32 oracle (b/<run>/final_Z_moved: 2.3 % and 5.6 % of the entries by
    # more than 1e-2): the product may differ from the reference in at most twice that share, and the typical entry by less than 1e-3.
    d = np.abs(z[:, :, ::8, ::8].cpu().numpy() - g[key + 'final_Z_sub'])
    ref_median, ref_share = g[key + 'final_Z_moved']
    print(name, 'final Z: median |dZ| %.2e (reference under perturbation %.2e), share > 1e-2 %.4f (%.4f)' % (np.median(d), ref_median, np.mean(d > 1e-2), ref_share))
    assert np.median(d) < 1e-3 and np.mean(d > 1e-2) <= 2 * ref_share, (float(np.median(d)), float(np.mean(d > 1e-2)))


def test_random_vgg_on_the_f7_sized_model(tmp_path):
    import models
    from esr_hip import pairmin
    from test_gpu_vgg import _weights_file
    from test_host_api import _opt
    from Z_optimization import Z_optimizer
    lat, B = 3, 3
    opt = _opt(nb=1, lat=lat, cem=True, is_train=False)
    opt['gpu_ids'] = [0]
    opt['path']['pretrained_model_F'] = _weights_file(tmp_path)
    m = models.create_model(opt, init_Fnet=True)
    fill_formula_weights(m.netG, gain=1.0)
    lr = seeded_uniform((1, 3, 24, 28), 920).to(DEV)
    z0 = seeded_uniform((B, lat, 96, 112), 921, -0.5, 0.5).to(DEV)
    m.feed_data({'LR': lr.expand(B, -1, -1, -1).clone(), 'Z': z0.clone()}, need_GT=False)
    m.test()
    zo = Z_optimizer(objective='random_VGG', Z_size=[96, 112], model=m, Z_range=1, max_iters=1, data={'LR': lr}, initial_LR=0.05, batch_size=B,
                     initial_Z=z0.clone())
    seen = []
    real = pairmin.random_share

    def spy(D, *a, **k):
        seen.append(D.detach().clone())
        return real(D, *a, **k)
    pairmin.random_share = spy
    try:
        z = zo.optimize()
    finally:
        pairmin.random_share = real
    assert len(zo.loss_values) == 1 and len(seen) == 1 and z.shape == z0.shape
    feats = seen[0]
    assert feats.dim() == 4 and feats.size(0) == B and float(feats.max()) > 1
    Zc, share = pairmin.random_share(feats.cpu(), clamp01=False)                # the CPU fallback on the same features
    np.testing.assert_allclose(zo.loss_values[0], float(share), rtol=1e-4)
    np.testing.assert_allclose(zo.latest_Z_loss_values, Zc.numpy(), rtol=1e-4)
    assert zo.Z_model.Z.grad is not None and float(zo.Z_model.Z.grad.abs().max()) > 0

"""GPU tests (-m gpu) of the pairwise KDE kernels (csrc/esr_kde.hip, esr_hip/kde.py) behind the patch-histogram and dictionary Z objectives:
SoftHistogramLoss against what the reference's own class computed (fixture tests/golden/patch_kde.npz, tools/gen_patch_kde_golden.py from
codes/Z_optimization.py:24-272), the kernels against a float64 torch restatement of the same formulas at a 256^2 region (where the reference's
[D, N, M] tensors no longer fit), and Z_optimizer's new objectives end to end."""
import os

import numpy as np
import pytest
import torch

from oracle.weights import fill_formula_weights, seeded_uniform
from oracle.zobj_contract_ref import _ref_cols, _ref_rows, _scores

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'patch_kde.npz')
CASES = {        # as tools/gen_patch_kde_golden.py::CASES
    'patchhist': (dict(patch_size=6, temperature=5e-4, dictionary_not_histogram=False, no_patch_DC=False), 'full', 'full'),
    'patchhist_noDC': (dict(patch_size=6, temperature=5e-4, dictionary_not_histogram=False, no_patch_DC=True), 'irr', 'full'),
    'patchdict_noDC': (dict(patch_size=6, temperature=1e-3, dictionary_not_histogram=True, no_patch_DC=True), 'full', 'full'),
    'patchdict_noDC_masked': (dict(patch_size=6, temperature=1e-3, dictionary_not_histogram=True, no_patch_DC=True), 'full', 'irr'),
    'dict_noDC': (dict(patch_size=1, temperature=1e-3, dictionary_not_histogram=True, no_patch_DC=True), 'full', 'full'),
}


@pytest.mark.parametrize('case', list(CASES))
def test_soft_histogram_loss_matches_the_reference(case):
    from Z_optimization import SoftHistogramLoss
    g = np.load(GOLDEN)
    cfg, dmask, imask = CASES[case]
    desired = torch.from_numpy(g['in/desired']).cuda()
    loss_fn = SoftHistogramLoss(bins=256, min=0, max=1, desired_hist_image=[desired], desired_hist_image_mask=[g['mask/' + dmask]],
                                input_im_HR_mask=torch.from_numpy(g['mask/' + imask]).cuda(), gray_scale=True, **cfg)
    if cfg['patch_size'] > 1:       # the de-duplicated bins: the same set, in the same (original patch) order
        want = g[case + '/bins']
        assert tuple(loss_fn.bins.shape) == want.shape
        np.testing.assert_allclose(loss_fn.bins.cpu().numpy(), want, rtol=0, atol=1e-6)
    cur = torch.from_numpy(g['in/cur']).cuda().requires_grad_(True)
    loss = loss_fn(cur)
    loss.sum().backward()
    np.testing.assert_allclose(loss.detach().double().cpu().numpy().reshape(-1), g[case + '/loss'], rtol=1e-4)
    want = g[case + '/grad']
    # dict_noDC (gray levels against 256 centres 1/255 apart at T = 1e-3) is almost flat: its exact gradient (~2e-8) is the near-total
    # cancellation of per-centre terms of size 2|d|/T/N ~ 0.1; an fp32 evaluation of those terms can only show it is ~0.
    atol = 2e-7 if case == 'dict_noDC' else 1e-5 * np.abs(want).max()
    np.testing.assert_allclose(cur.grad.double().cpu().numpy(), want, rtol=2e-3, atol=atol)


# ---------------------------------------------------------------------------------------------- float64 restatement of the formulas
def _region_patches(seed, side, overlap, no_dc=True, noise=0.0, base=None):
    from esr_hip import kde
    idx = torch.from_numpy(kde.patch_extraction_indexes(np.ones((side, side)), 6, overlap)).cuda()
    if base is None:
        coarse = seeded_uniform((1, 1, side // 8, side // 8), seed).cuda()
        base = torch.nn.functional.interpolate(coarse, size=(side, side), mode='bilinear', align_corners=True)[0, 0]
    img = (base + noise * (seeded_uniform((side, side), seed + 1).cuda() - 0.5)).clamp(0, 1)
    p = img.reshape(-1)[idx]
    return (p - p.mean(1, keepdim=True) if no_dc else p).contiguous(), base


def _check_grad(got, ref):
    ref = ref.cpu().numpy()
    np.testing.assert_allclose(got.double().cpu().numpy(), ref, rtol=2e-3, atol=1e-5 * np.abs(ref).max())


def test_kde_kernels_at_a_256_region_match_float64():
    """256^2 region: N = 3612 patches (overlap 0.5) of a noisy image against the de-duplicated patches of the clean one (overlap 30/36):
    row mode (dictionary, T = 1e-3) and column mode (KDE histogram, T = 5e-4), values and gradients, against float64."""
    from esr_hip import kde
    X, base = _region_patches(1400, 256, 0.5, noise=0.05)
    D, _ = _region_patches(1400, 256, 30 / 36, base=base)
    assert X.shape == (3612, 36) and D.shape[0] == 10917
    bins = D[kde.dedup_keep(D, 1 / 510)].contiguous()
    g = seeded_uniform((X.size(0),), 1402, 0.5, 1.5).cuda().double()
    Xa = X.clone().requires_grad_(True)
    lse = kde.row_lse(Xa, bins, 1e-3, 1.0)
    (lse * g).sum().backward()
    ref, gref = _ref_rows(X, bins, 1e-3, g)
    np.testing.assert_allclose(lse.detach().cpu().numpy(), ref.cpu().numpy(), rtol=1e-5, atol=1e-4)
    _check_grad(Xa.grad, gref)
    gc = seeded_uniform((1, bins.size(0)), 1403, -1.0, 1.0).cuda().double()
    Xa = X.clone().requires_grad_(True)
    lse = kde.column_lse(Xa, (X.size(0),), bins, 5e-4, 1.0)
    (lse * gc).sum().backward()
    ref, gref = _ref_cols(X, (X.size(0),), bins, 5e-4, gc)
    np.testing.assert_allclose(lse.detach().cpu().numpy(), ref.cpu().numpy(), rtol=1e-5, atol=1e-3)
    _check_grad(Xa.grad, gref)


def test_far_patches_stay_finite_in_the_log_domain():
    """DC-free patches far from every bin at T = 1e-3 (s/T ~ 160-200: exp(-s/T) is below fp32's range, a plain fp32 sum would be 0 and its
    log -inf); the row and column log sums and the row gradient must be finite and equal float64's log-sum-exp."""
    from esr_hip import kde
    # opposite DC-free +-0.21 patterns with a little noise: every coordinate difference lies in [0.34, 0.495], far, yet clear of the wrap's
    # switch at 0.5 (where fp32 and float64 may take branches of opposite derivative sign)
    pattern = (torch.arange(36) % 2 * 0.42 - 0.21).cuda()
    X = -pattern + 0.06 * (seeded_uniform((1500, 36), 1410).cuda() - 0.5)
    X = X - X.mean(1, keepdim=True)
    B = pattern + 0.06 * (seeded_uniform((900, 36), 1411).cuda() - 0.5)
    B = B - B.mean(1, keepdim=True)
    sT = _scores(X.double(), B.double()) / 1e-3
    assert float(sT.min()) > 150 and float(sT.max()) < 250
    g = torch.ones(X.size(0), dtype=torch.float64, device='cuda')
    Xa = X.clone().requires_grad_(True)
    lse = kde.row_lse(Xa, B, 1e-3, 1.0)
    lse.sum().backward()
    assert torch.isfinite(lse).all() and torch.isfinite(Xa.grad).all()
    ref, gref = _ref_rows(X, B, 1e-3, g)
    np.testing.assert_allclose(lse.detach().cpu().numpy(), ref.cpu().numpy(), rtol=1e-5)
    _check_grad(Xa.grad, gref)
    col = kde.column_lse(X, (X.size(0),), B, 1e-3, 1.0)
    ref, _ = _ref_cols(X, (X.size(0),), B, 1e-3, torch.zeros(1, B.size(0), dtype=torch.float64, device='cuda'))
    assert torch.isfinite(col).all()
    np.testing.assert_allclose(col.cpu().numpy(), ref.cpu().numpy(), rtol=1e-5)


def test_a_batch_of_images_with_different_masks():
    """Column mode over a batch whose images have different point counts (different masks): one launch, per-image sums; and the
    wrap at |δ| > 1 (DC-free values against bins with a DC offset)."""
    from esr_hip import kde
    counts = (700, 257, 1, 1200)
    X = (seeded_uniform((sum(counts), 9), 1420, -1.0, 1.0)).cuda()
    B = seeded_uniform((600, 9), 1421, -0.2, 1.0).cuda()
    gc = seeded_uniform((len(counts), 600), 1422, -1.0, 1.0).cuda().double()
    Xa = X.clone().requires_grad_(True)
    lse = kde.column_lse(Xa, counts, B, 0.05, 1.0)
    (lse * gc).sum().backward()
    ref, gref = _ref_cols(X, counts, B, 0.05, gc)
    np.testing.assert_allclose(lse.detach().cpu().numpy(), ref.cpu().numpy(), rtol=1e-5, atol=1e-5)
    _check_grad(Xa.grad, gref)
    # the same images through SoftHistogramLoss: masks differ per image only through patch selection, so check the dedup kernel too
    keep = kde.dedup_keep(B, 0.3).cpu().numpy()
    Bd = B.cpu().double()
    close = ((Bd[:, None, :] - Bd[None]).abs() < 0.3).all(2)
    want = ~torch.triu(close, diagonal=1).any(1).numpy()
    np.testing.assert_array_equal(keep, want)


def test_kernel_gradients_match_finite_differences_in_double():
    """Tiny case: central differences of the float64 restatement (h = 1e-6) against the kernels' gradients, both modes."""
    from esr_hip import kde
    X = (seeded_uniform((20, 4), 1430, -1.0, 1.0)).cuda()
    B = seeded_uniform((30, 4), 1431).cuda()
    T = 0.05
    gr = seeded_uniform((20,), 1432, 0.5, 1.5).cuda().double()
    gc = seeded_uniform((2, 30), 1433, -1.0, 1.0).cuda().double()

    def f_rows(x):
        return (torch.logsumexp(-_scores(x, B.double()) / T, 1) * gr).sum()

    def f_cols(x):
        s = -_scores(x, B.double()) / T
        return (torch.stack([torch.logsumexp(s[:12], 0), torch.logsumexp(s[12:], 0)]) * gc).sum()

    for f, run in ((f_rows, lambda xa: (kde.row_lse(xa, B, T, 1.0) * gr).sum()),
                   (f_cols, lambda xa: (kde.column_lse(xa, (12, 8), B, T, 1.0) * gc).sum())):
        xa = X.clone().requires_grad_(True)
        run(xa).backward()
        xd = X.double()
        fd = torch.zeros_like(xd)
        h = 1e-6
        for i in range(xd.size(0)):
            for d in range(xd.size(1)):
                e = torch.zeros_like(xd)
                e[i, d] = h
                fd[i, d] = (f(xd + e) - f(xd - e)) / (2 * h)
        np.testing.assert_allclose(xa.grad.double().cpu().numpy(), fd.cpu().numpy(), rtol=1e-3, atol=1e-4 * float(fd.abs().max()))


# ---------------------------------------------------------------------------------------------- Z_optimizer end to end
@pytest.mark.parametrize('objective', ['patchdict_noDC', 'patchhist'])
def test_z_optimizer_patch_objectives_in_a_region(objective):
    import models
    from Z_optimization import Z_optimizer
    from test_gpu_callers_f7 import product_opt
    m = models.create_model(product_opt(False))
    fill_formula_weights(m.netG, gain=0.5)
    lr = seeded_uniform((1, 3, 24, 28), 920).to(m.device)
    B = 2
    z0 = seeded_uniform((B, 3, 96, 112), 921, -0.3, 0.3).to(m.device)
    im_mask = np.zeros([96, 112], dtype=np.float32); im_mask[24:72, 32:96] = 1
    z_mask = np.zeros([96, 112], dtype=np.float32); z_mask[16:80, 24:104] = 1
    m.feed_data({'LR': lr.expand(B, -1, -1, -1).clone(), 'Z': z0.clone()}, need_GT=False)
    m.test()
    desired = (m.fake_H[:1].detach().clamp(0, 1) * 0.6 + 0.2)          # a lower-contrast version of the current output
    zo = Z_optimizer(objective=objective, Z_size=[96, 112], model=m, Z_range=1, max_iters=4, initial_Z=z0.clone(), initial_LR=0.1, batch_size=B,
                     data={'LR': lr.expand(B, -1, -1, -1).clone(), 'desired': [desired], 'Desired_Im_Mask': None}, image_mask=im_mask, Z_mask=z_mask)
    z = zo.optimize()
    assert torch.isfinite(z).all()
    assert all(np.isfinite(zo.loss_values)) and min(zo.loss_values) < zo.loss_values[0]
    outside = torch.from_numpy(z_mask == 0).to(z.device).expand_as(z)
    assert float((z - z0)[outside].abs().max()) < 1e-6 and float((z - z0).abs().max()) > 1e-4

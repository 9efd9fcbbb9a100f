"""Pins oracle/zobj_contract_ref.py, the float64 restatement that tests/test_gpu_zobj_contract.py holds the Z-objective kernels to, and what
those entry points refuse - all without a GPU:
  * the restatement reproduces the function-level values of the reference's fixtures (soft_histogram.npz, filter_loss.npz, local_z.npz,
    special_z.npz, scribble.npz, random_z.npz, patch_kde.npz) to the tolerance each fixture's own test uses - the periodicity and Plus
    losses among them, which are what pins the shifted-L1 restatement (on the wrapper's taps, whose ranges must contain the tight ones);
  * its autograd gradients equal the closed forms written in include/esr_hip.h (the coef forms of esr_img_stats_grad, the a[p] (v - mean[p]) form
    of the patch STD, the gather form of the patch magnitude);
  * the comparator accepts the reference rounded to fp32 and rejects a planted error per entry point, each with that case's own bound;
  * the inputs of the GPU file stay inside the tie caps by the float64 reference alone (they are generated on the CPU, so this is the place);
  * every ESR_E_ARG / ESR_E_UNSUPPORTED of these entry points, on buffers large enough for the correct call (device memory when a GPU is
    visible, host memory otherwise: then a missing refusal shows as a failed launch, not as ESR_OK); the unmodified call is shown not to be
    refused, and the outputs keep their fill after a refusal."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import test_gpu_zobj_contract as G
from oracle import zobj_contract_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
U = R.U
E_ARG, E_UNSUPPORTED = -1, -2


def rejects(got, ref, bound, what=''):
    with pytest.raises(AssertionError):
        R.compare(got, ref, bound, what)
    return True


def r32(t):
    return t.float().double()


# =================================================================================================== fixtures
def test_soft_histogram_fixture():
    from oracle.weights import seeded_uniform
    g = np.load(os.path.join(GOLDEN, 'soft_histogram.npz'))
    gray = seeded_uniform((1, 3, 40, 36), 1101)[0].mean(0).reshape(-1)
    h = R.soft_hist(gray, 64, 0.0, 1.0, 2e-3, 1e-7)
    h = (h / h.sum()).view(1, -1)                                # the reference normalises the histogram to sum 1
    for name in ('plain', 'masked'):
        np.testing.assert_allclose(h.numpy(), g[name + '/desired_hist'], rtol=1e-4, atol=1e-8)


@pytest.mark.parametrize('name', ['plain', 'masked'])
def test_soft_histogram_fixture_loss(monkeypatch, name):
    """SoftHistogramLoss (the KL divergence of the normalised histograms) with the wrapper replaced by the restatement, float64 autograd"""
    from esr_hip import zobj
    from oracle.weights import seeded_uniform
    from Z_optimization import SoftHistogramLoss
    monkeypatch.setattr(zobj, 'soft_histogram', lambda v, K, lo, hi, T, eps=1e-7: R.soft_hist(v, int(K), lo, hi, T, eps) / v.numel())
    g = np.load(os.path.join(GOLDEN, 'soft_histogram.npz'))
    mask = torch.from_numpy(g['masked/mask']) if name == 'masked' else None
    loss_fn = SoftHistogramLoss(bins=64, min=0, max=1, desired_hist_image=[seeded_uniform((1, 3, 40, 36), 1101)], desired_hist_image_mask=[None],
                                input_im_HR_mask=mask, gray_scale=True, patch_size=1, temperature=2e-3)
    np.testing.assert_allclose(loss_fn.desired_hists_list[0].numpy(), g[name + '/desired_hist'], rtol=1e-4, atol=1e-8)
    cur = (seeded_uniform((2, 3, 40, 36), 1102) ** 2).requires_grad_(True)
    loss = loss_fn(cur)
    loss.backward()
    assert abs(float(loss.detach()) - float(g[name + '/loss'])) < 1e-3 * float(g[name + '/loss'])
    np.testing.assert_allclose(cur.grad.numpy(), g[name + '/grad'], rtol=2e-3, atol=2e-7)


def test_local_z_fixture_patch_std():
    from esr_hip import local
    g = np.load(os.path.join(GOLDEN, 'local_z.npz'))
    x = torch.from_numpy(g['a/x'])
    corners = torch.from_numpy(local.patch_corners(g['a/mask']))
    sel = corners.flatten() != 0
    S, _ = R.patch_std(x, corners)
    np.testing.assert_allclose(S.reshape(x.size(0), -1)[:, sel].t().numpy(), g['a/std/S'], rtol=1e-5, atol=1e-7)
    dS = torch.zeros(x.size(0), sel.numel(), dtype=torch.float64)
    dS[:, sel] = torch.from_numpy(g['a/std/cot']).double().t()
    grad, _, _ = R.patch_std_grad(x, corners, dS.reshape(S.shape))
    np.testing.assert_allclose(grad.numpy(), g['a/std/grad'], rtol=1e-5, atol=1e-5 * np.abs(g['a/std/grad']).max())


def _periodicity(x, mask, points, interpolated):
    """sum over the period points of mean_{c,i,j} M |GS+ - GS-| -> [B], from the restatement on the wrapper's taps (host code); the wrapper's
    ranges must contain the tight ones"""
    from esr_hip import local
    H, W = mask.shape
    tot = 0
    for p in points:
        pr = local.ShiftPair(p, H, W, interpolated=interpolated)
        bx, fx, by, fy = [torch.from_numpy(np.asarray(a)) for a in (pr.base_x, pr.frac_x, pr.base_y, pr.frac_y)]
        tot = tot + R.shift_l1(x, mask, bx, fx, by, fy).sum(1) / (x.size(1) * pr.ny * pr.nx)
        for tight, given in ((R.tight_ranges(bx, pr.nx, W), pr.ranges_x), (R.tight_ranges(by, pr.ny, H), pr.ranges_y)):
            given = torch.from_numpy(np.asarray(given))
            some = tight[..., 1] > tight[..., 0]
            assert bool((given[..., 0][some] <= tight[..., 0][some]).all()) and bool((given[..., 1][some] >= tight[..., 1][some]).all())
    return tot


@pytest.mark.parametrize('case', ['nonint1', 'nonint2', 'int1'])
def test_local_z_fixture_periodicity(case):
    from esr_hip import local
    g = np.load(os.path.join(GOLDEN, 'local_z.npz'))
    mask = torch.from_numpy(g['a/mask'])
    corners = torch.from_numpy(local.patch_corners(g['a/mask']))
    sel = (corners != 0)[None]
    x = torch.from_numpy(g['a/x']).double().requires_grad_(True)
    S = R.patch_std(x, corners)[0]
    initial = R.patch_std(x[:1].detach(), corners)[0]
    np.testing.assert_allclose(initial[sel].numpy(), g['a/%s/initial_STD' % case].reshape(-1), rtol=1e-5, atol=1e-7)
    n_sel = int(sel.sum()) * x.size(0)
    loss = (20 * (S - initial) ** 2 * sel).sum() / n_sel + _periodicity(x, mask.double(), g['a/%s/points' % case], 'nonint' in case)
    np.testing.assert_allclose(loss.detach().numpy(), g['a/%s/loss' % case], rtol=1e-5)
    loss.sum().backward()
    gr = g['a/%s/grad' % case]
    np.testing.assert_allclose(x.grad.numpy(), gr, rtol=1e-5, atol=1e-5 * np.abs(gr).max())


@pytest.mark.parametrize('case', ['nonint1', 'nonint2', 'whole'])
def test_special_z_fixture_plus(case):
    from esr_hip import local
    g = np.load(os.path.join(GOLDEN, 'special_z.npz'))
    mask = torch.from_numpy(g['a/mask']).double()
    I0 = torch.from_numpy(g['a/x_init']).double()
    x = torch.from_numpy(g['a/x']).double().requires_grad_(True)
    if case != 'whole':
        corners = torch.from_numpy(local.patch_corners(g['a/mask']))
        sel = corners != 0
        std = lambda im: R.patch_std(im, corners)[0][:, sel].t()  # noqa: E731      [P, B]
    else:
        def std(im):                                             # the masked STD from the kind 0 sums
            s = R.img_stats(im, mask, 1, 0)
            n = im[0].numel()
            return ((s[:, 1] - s[:, 0] ** 2 / n) / (n - 1)).sqrt().view(1, -1)
    desired = std(I0).detach() + 0.03
    np.testing.assert_allclose(desired.numpy(), g['a/plus/%s/desired_STD' % case], rtol=1e-5, atol=1e-7)
    loss = _periodicity(x, mask, g['a/plus/%s/points' % case], True) + (20 * (std(x) - desired) ** 2).mean()
    np.testing.assert_allclose(loss.detach().numpy(), g['a/plus/%s/loss' % case], rtol=1e-5)
    loss.sum().backward()
    gr = g['a/plus/%s/grad' % case]
    np.testing.assert_allclose(x.grad.numpy(), gr, rtol=1e-5, atol=1e-5 * np.abs(gr).max())


@pytest.mark.parametrize('sign', ['increase', 'decrease'])
def test_special_z_fixture_patch_mag(sign):
    g = np.load(os.path.join(GOLDEN, 'special_z.npz'))
    x = torch.from_numpy(g['a/x'])
    H, W = g['a/mask'].shape
    first = g['a/mag/%s/patches' % sign][:, 0]                   # flat index of every window's first pixel
    P = first.shape[0]
    ci = torch.full((H - 6, W - 6), -1, dtype=torch.int32)
    ci[torch.from_numpy(first // W), torch.from_numpy(first % W)] = torch.arange(P, dtype=torch.int32)
    desired = torch.from_numpy(g['a/mag/%s/desired' % sign]).t().contiguous()          # [P][49]
    loss = R.patch_mag(x, ci, desired, P) / (49.0 * P)
    np.testing.assert_allclose(loss.numpy(), g['a/mag/%s/loss' % sign], rtol=1e-5)
    grad, _, _ = R.patch_mag_grad(x, ci, desired, P, torch.ones(x.size(0)))
    gr = g['a/mag/%s/grad' % sign]
    np.testing.assert_allclose(grad.numpy(), gr, rtol=1e-5, atol=1e-5 * np.abs(gr).max())


def test_scribble_fixture():
    from esr_hip import scribble
    g = np.load(os.path.join(GOLDEN, 'scribble.npz'))
    I0 = torch.clamp(torch.from_numpy(g['a/x_init']), 0, 1)
    spec = scribble.ScribbleSpec(g['a/scribble'], g['a/mask'], g['a/D'], constraint=True, initial=I0)        # the label map is host code
    x = torch.from_numpy(g['a/x'])
    B, Cc, H, W = x.shape
    lab, D = torch.from_numpy(np.asarray(spec.labels)), spec.desired[0]
    i0 = spec.initial.expand(B, -1, -1, -1)
    p = R.scribble(x, D, lab, i0)
    L = (p[:, :4] * R.scribble_weights(Cc, H, W)).sum(1)
    np.testing.assert_allclose(L.numpy(), g['a/loss'], rtol=1e-5)
    norm = B * Cc * H * W
    np.testing.assert_allclose(float(p[:, 4].sum()) / norm, float(g['a/constraint']), rtol=1e-5)
    for key, gb, g_con in (('a/grad_loss', torch.ones(B), 0.0), ('a/grad_constraint', torch.zeros(B), 1.0 / norm)):
        grad, _ = R.scribble_grad(x, D, lab, i0, gb, g_con)
        gr = g[key]
        np.testing.assert_allclose(grad.numpy(), gr, rtol=1e-5, atol=1e-5 * np.abs(gr).max())


@pytest.mark.parametrize('code', ['SVDinNormedOut_structure_tensor', 'structure_tensor'])
def test_filter_loss_fixture(monkeypatch, code):
    """FilterLoss with its structure tensor taken from the restatement's kind 2 sums (over C (H - 1) (W - 1)), on the fixture's three calls"""
    from models.modules.loss import FilterLoss
    from oracle.weights import seeded_uniform
    g = np.load(os.path.join(GOLDEN, 'filter_loss.npz'))

    def tensor(x):
        n = x.size(1) * (x.size(2) - 1) * (x.size(3) - 1)
        return (R.img_stats(x, None, 0, 2) / n).t().to(x.dtype)
    monkeypatch.setattr(FilterLoss, 'structure_tensor', staticmethod(tensor))
    fl = FilterLoss(latent_channels=code)
    for call in range(3):
        sr = seeded_uniform((4, 3, 24, 20), 1000 + call).requires_grad_(True)
        hr = seeded_uniform((4, 3, 24, 20), 1010 + call)
        z = seeded_uniform((4, 3, 1, 1), 1020 + call, -1.0, 1.0) * torch.ones(4, 3, 24, 20)
        loss = fl({'SR': sr, 'HR': hr, 'Z': z})
        np.testing.assert_allclose(loss.detach().numpy(), g['%s/call%d' % (code, call)], rtol=1e-4, atol=5e-7)
    loss.sum().backward()
    np.testing.assert_allclose(sr.grad.numpy(), g[code + '/dSR'], rtol=2e-4, atol=1e-7)


PATCH_KDE = {        # as tests/test_gpu_kde.py::CASES
    'patchhist': (dict(patch_size=6, temperature=5e-4, dictionary_not_histogram=False, no_patch_DC=False), 'full', 'full'),
    'patchhist_noDC': (dict(patch_size=6, temperature=5e-4, dictionary_not_histogram=False, no_patch_DC=True), 'irr', 'full'),
    'patchdict_noDC': (dict(patch_size=6, temperature=1e-3, dictionary_not_histogram=True, no_patch_DC=True), 'full', 'full'),
    'patchdict_noDC_masked': (dict(patch_size=6, temperature=1e-3, dictionary_not_histogram=True, no_patch_DC=True), 'full', 'irr'),
    'dict_noDC': (dict(patch_size=1, temperature=1e-3, dictionary_not_histogram=True, no_patch_DC=True), 'full', 'full'),
}


@pytest.mark.parametrize('case', list(PATCH_KDE))
def test_patch_kde_fixture(monkeypatch, case):
    """SoftHistogramLoss with the three KDE wrappers replaced by the restatement's log-sums (float64 autograd) and de-duplication"""
    from esr_hip import kde
    from Z_optimization import SoftHistogramLoss

    def col(X, counts, bins, T, period):
        out, r = [], 0
        for n in counts:
            out.append(R.kde_fwd_graph(bins, X[r:r + n], period, T))
            r += n
        return torch.stack(out)
    monkeypatch.setattr(kde, 'column_lse', col)
    monkeypatch.setattr(kde, 'row_lse', lambda X, bins, T, period: R.kde_fwd_graph(X, bins, period, T))
    monkeypatch.setattr(kde, 'dedup_keep', lambda b, hw: R.kde_dedup(b, hw).bool())
    g = np.load(os.path.join(GOLDEN, 'patch_kde.npz'))
    cfg, dmask, imask = PATCH_KDE[case]
    loss_fn = SoftHistogramLoss(bins=256, min=0, max=1, desired_hist_image=[torch.from_numpy(g['in/desired'])], desired_hist_image_mask=[g['mask/' + dmask]],
                                input_im_HR_mask=torch.from_numpy(g['mask/' + imask]), gray_scale=True, **cfg)
    if cfg['patch_size'] > 1:
        np.testing.assert_allclose(loss_fn.bins.numpy(), g[case + '/bins'], rtol=0, atol=1e-6)
    cur = torch.from_numpy(g['in/cur']).requires_grad_(True)
    loss = loss_fn(cur)
    loss.sum().backward()
    np.testing.assert_allclose(loss.detach().double().numpy().reshape(-1), g[case + '/loss'], rtol=1e-4)
    want = g[case + '/grad']
    atol = 2e-7 if case == 'dict_noDC' else 1e-5 * np.abs(want).max()
    np.testing.assert_allclose(cur.grad.double().numpy(), want, rtol=2e-3, atol=atol)


def test_random_z_fixture_pairmin():
    g = np.load(os.path.join(GOLDEN, 'random_z.npz'))
    cases = sorted({k.rsplit('/', 1)[0] for k in g.files if k.startswith('a/B') and k.endswith('/x')})
    assert len(cases) == 12
    for key in cases:
        x = torch.from_numpy(g[key + '/x'])
        mask = torch.from_numpy(g['a/mask']) if '_m1' in key else None
        init = torch.from_numpy(g[key + '/init']) if '_l1' in key else None
        B, n = x.size(0), x[0].numel()
        s, _ = R.pairmin(x, 0, B, 1, mask, init, 0.3)
        np.testing.assert_allclose((-s / n).numpy(), g[key + '/Z_loss'], rtol=1e-5, atol=1e-7, err_msg=key)
        grad, tie = R.pairmin_grad(x, 0, B, 1, mask, init, 0.3, -1.0 / (n * B))
        gr = g[key + '/grad']
        ok = ~tie[None].expand_as(grad).numpy()
        assert tie.double().mean() <= R.PAIRMIN_TIE_CAP
        np.testing.assert_allclose(grad.numpy()[ok], gr[ok], rtol=1e-5, atol=1e-5 * max(np.abs(gr).max(), 1e-12), err_msg=key)


# =================================================================================================== gradients: autograd == the header's closed forms
@pytest.mark.parametrize('shape,Cc', [('h1', 1), ('w1', 3), ('rag', 1), ('rag', 3), ('tail', 1)])
def test_img_stats_gradients_are_the_closed_forms(shape, Cc):
    x, mask, coef = G.img_case(shape, Cc)
    for kind in (0, 1, 2):
        for m in (None, mask):
            for clamp01 in (0, 1):
                g, mag = R.img_stats_grad(x, m, clamp01, kind, coef)
                c = R.img_stats_grad_closed(x, m, clamp01, kind, coef)
                assert float((g - c).abs().max()) <= 1e-13 * max(1.0, float(c.abs().max())), (kind, clamp01)
                assert bool((g.abs() <= mag * (1 + 1e-12) + 1e-300).all()), 'mag does not bound the gradient'
    # the sums are what _ref_stats (the older test's torch expressions) normalises
    s = R.img_stats(x, mask, 1, 0)
    n = x[0].numel()
    std = ((s[:, 1] - s[:, 0] ** 2 / n) / (n - 1)).sqrt()
    if n > 1:
        np.testing.assert_allclose(std.numpy(), R._ref_stats(x, mask, 1, 0).numpy(), rtol=1e-9)


@pytest.mark.parametrize('H,W', G.PATCH_SHAPES)
def test_patch_gradients_are_the_gather_forms(H, W):
    x, corners = G.patch_case(3, H, W)
    dS = torch.randn(2, H - 6, W - 6, generator=G.rng(1))
    g, mag_a, mag_t = R.patch_std_grad(x, corners, dS)
    c = R.patch_std_grad_closed(x, corners, dS)
    assert float((g - c).abs().max()) <= 1e-12 * max(1.0, float(c.abs().max()))
    assert bool((g.abs() <= mag_t * (1 + 1e-9) + 1e-300).all())
    ci, desired = G.mag_case(H, W, 5)
    gb = torch.tensor([0.7, -1.3])
    g, mag_n, mag_t = R.patch_mag_grad(x, ci, desired, 5, gb)
    v = torch.clamp(x.double(), 0, 1).mean(1)
    dv = torch.zeros_like(v)
    for cy, cx, p in R._selected(ci, 5):                        # the header's gather form, written as its scatter
        dv[:, cy:cy + 7, cx:cx + 7] += v[:, cy:cy + 7, cx:cx + 7] - desired[p].double().reshape(7, 7)
    c = (2 * gb.double() / (49 * 5))[:, None, None, None] * dv[:, None] / 3 * ((x >= 0) & (x <= 1))
    assert float((g - c).abs().max()) <= 1e-13
    assert bool((g.abs() <= mag_t * (1 + 1e-9) + 1e-300).all())


# =================================================================================================== the comparator and the planted errors
def test_comparator_basics():
    ref = torch.tensor([1.0, -2.0, 0.0], dtype=torch.float64)
    assert R.compare(ref.float(), ref, U * ref.abs()) <= 1.0
    rejects(torch.tensor([1.0, float('nan'), 0.0]), ref, torch.full((3,), float('inf')))
    rejects(torch.tensor([1.0, -2.0, 1e-30]), ref, U * ref.abs())
    rejects(torch.tensor([1.0, -2.0]), ref, 1.0)


def test_planted_img_stats():
    x, mask, coef = G.img_case('rag', 3)
    base = torch.randn(x.shape, generator=G.rng(2)) + 0.25
    for kind in (0, 1, 2):
        ref, mag = R.img_stats(x, mask, 1, kind, with_mag=True)
        bound = 12 * U * mag
        live = 3 if kind == 2 else 2
        assert R.compare(r32(ref)[:, :live], ref[:, :live], bound[:, :live]) <= 1
        rejects(R.img_stats(x, None, 1, kind)[:, :live], ref[:, :live], bound[:, :live], 'the mask left out')
        rejects(R.img_stats(x, mask, 0, kind)[:, :live], ref[:, :live], bound[:, :live], 'no clamp')
        g, gmag = R.img_stats_grad(x, mask, 1, kind, coef)
        gb = 12 * U * gmag
        assert R.compare(r32(g), g, gb) <= 1
        want, b1 = R.accumulated(base, g)
        assert R.compare(r32(want), want, gb + b1) <= 1
        rejects(g, want, gb + b1, 'accumulate ignored')
        rejects(want, g, gb, 'accumulate applied when it is 0')
        # the clamp gate made exclusive at 0 and 1
        excl = g * ((x > 0) & (x < 1))
        assert bool(((x == 0) | (x == 1)).any())
        rejects(excl, g, gb, 'exclusive gate')
    x1, _, c1 = G.img_case('rag', 1)
    ref, mag = R.img_stats(x1, None, 1, 2, with_mag=True)
    three = R.img_stats(x1.expand(-1, 3, -1, -1), None, 1, 2)
    rejects(three, ref, 12 * U * mag, 'C = 1 read as three channels')


def test_planted_soft_hist():
    n, K, lo, hi = G.HIST_CASES[3]
    v, gh = G.hist_case(n, K, lo, hi)
    T, eps = G.f32(5e-4), G.f32(1e-7)
    ref = R.soft_hist(v, K, lo, hi, T, eps)
    bound = R.rtol_bound(ref, 1e-5)
    assert R.compare(r32(ref), ref, bound) <= 1
    drop = ref.clone()
    drop[256:] = 0
    rejects(drop, ref, bound, 'bins >= 256 dropped')
    rejects(R.soft_hist(v, K, lo, hi, T, eps, period=hi - lo), ref, bound, 'the wrap period taken as hi - lo')
    rejects(R.soft_hist(v[:4096], K, lo, hi, T, eps), ref, bound, 'the ragged last slab dropped')
    g = R.soft_hist_grad(v, K, lo, hi, T, eps, gh)
    gbound = R.rtol_bound(g, 1e-3, 1e-5)
    assert R.compare(r32(g), g, gbound) <= 1
    gd = gh.clone()
    gd[256:] = 0
    rejects(R.soft_hist_grad(v, K, lo, hi, T, eps, gd), g, gbound, 'bins >= 256 dropped in the backward')


def test_planted_patch():
    x, corners = G.patch_case(1, 23, 71)
    S, M = R.patch_std(x, corners)
    bound = U * (26 * S + 60)
    assert R.compare(r32(S), S, bound) <= 1 and R.compare(r32(M), M, bound) <= 1
    rejects(M / 3, M, bound, 'the channel mean taken over 3 when C = 1')
    rejects(S * (48.0 / 49.0) ** 0.5, S, bound, 'the biased std')
    dS = torch.randn(2, 17, 65, generator=G.rng(3))
    g, mag_a, mag_t = R.patch_std_grad(x, corners, dS)
    gb = U * (56 * mag_t + 4 * mag_a).expand_as(g)
    base = torch.randn(x.shape, generator=G.rng(4)) + 0.25
    want, b1 = R.accumulated(base, g)
    assert R.compare(r32(g), g, gb) <= 1 and R.compare(r32(want), want, gb + b1) <= 1
    rejects(g, want, gb + b1, 'accumulate ignored')
    rejects(want, g, gb, 'accumulate applied when it is 0')
    rejects(g / 3, g, gb, 'dx divided by 3 when C = 1')
    ci, desired = G.mag_case(23, 71, 5)
    ref, s1 = R.patch_mag(x, ci, desired, 5, with_mag=True)
    pb = U * (52 * ref + 4 * s1)
    assert R.compare(r32(ref), ref, pb) <= 1
    wrong = ci.clone()
    wrong[ci == 5] = 4
    rejects(R.patch_mag(x, wrong, desired, 5), ref, pb, 'ordinal P read as selected')
    gm, mag_n, mag_t = R.patch_mag_grad(x, ci, desired, 5, torch.tensor([0.7, -1.3]))
    mb = U * (56 * mag_t + 2 * mag_n).expand_as(gm)
    want, b1 = R.accumulated(base, gm)
    assert R.compare(r32(gm), gm, mb) <= 1
    rejects(gm, want, mb + b1, 'accumulate ignored')
    rejects(want, gm, mb, 'accumulate applied when it is 0')
    rejects(R.patch_mag_grad(x, wrong, desired, 5, torch.tensor([0.7, -1.3]))[0], gm, mb, 'ordinal P read as selected')


def test_planted_shift_l1():
    x, mask, bx, fx, by, fy, g = G.shift_case(3, 290, 7, True)
    ref, mag = R.shift_l1(x, mask, bx, fx, by, fy, with_mag=True)
    bound = 23 * U * mag
    assert R.compare(r32(ref), ref, bound) <= 1
    rejects(R.shift_l1(x, mask, bx[:, :256], fx[:, :256], by, fy), ref, bound, 'output columns >= 256 dropped')
    gr, gmag, cnt, tie = R.shift_l1_grad(x, mask, bx, fx, by, fy, g)
    gb = (cnt + 16) * U * gmag
    gb[tie] = float('inf')
    assert R.compare(r32(gr), gr, gb) <= 1
    rejects(R.shift_l1_grad(x, mask, bx[:, :256], fx[:, :256], by, fy, g)[0], gr, gb, 'output columns >= 256 dropped')
    base = torch.randn(x.shape, generator=G.rng(5)) + 0.25
    want, b1 = R.accumulated(base, gr)
    rejects(gr, want, gb + b1, 'accumulate ignored')
    rejects(want, gr, gb, 'accumulate applied when it is 0')
    # tight ranges name exactly the outputs whose taps touch a source column
    rx = R.tight_ranges(bx, 290, G.SH_W)
    for s in (0, 1):
        for src in (0, 150, 299):
            hit = [j for j in range(290) if int(bx[s, j]) in (src, src - 1)]
            assert (int(rx[s, src, 0]), int(rx[s, src, 1])) == ((hit[0], hit[-1] + 1) if hit else (0, 0))


def test_planted_scribble():
    x, D, lab, i0, g = G.scribble_case(3, 6, 257)
    ref = R.scribble(x, D, lab, i0)
    bound = 4 * U * ref
    assert R.compare(r32(ref), ref, bound) <= 1
    rejects(R.scribble(x, D, lab & 0xBF, i0), ref, bound, 'bit 6 ignored with i0 given')
    l31 = torch.where((lab & 0x3f) == 63, (lab & 0xC0) | 2, lab)
    rejects(R.scribble(x, D, l31, i0), ref, bound, 'region id 63 taken for its neighbour 2')
    gr, gmag = R.scribble_grad(x, D, lab, i0, g, 0.35)
    gb = (14 * U * gmag).expand_as(gr)
    assert R.compare(r32(gr), gr, gb) <= 1
    rejects(R.scribble_grad(x, D, lab, i0, g, 0.0)[0], gr, gb, 'g_con dropped')
    rejects(R.scribble_grad(x, D, lab, i0.flip(0), g, 0.35)[0], gr, gb, 'i0 of the other image')
    base = torch.randn(x.shape, generator=G.rng(6)) + 0.25
    want, b1 = R.accumulated(base, gr)
    rejects(gr, want, gb + b1, 'accumulate ignored')
    rejects(want, gr, gb, 'accumulate applied when it is 0')
    for H, W in ((1, 300), (5, 1)):
        w = R.scribble_weights(3, H, W)
        assert float(w[1]) == 0 and (float(w[2]) == 0) == (H == 1) and (float(w[3]) == 0) == (W == 1)


def test_planted_pairmin():
    x, mask, init = G.pair_case('stride-sub')
    n = x[0].numel()
    ref, mag = R.pairmin(x, 1, 3, 1, mask, init, 0.4)
    bound = 5 * U * mag
    assert R.compare(r32(ref), ref, bound) <= 1
    e = torch.arange(n)
    rejects(R.pairmin(x, 1, 3, 1, mask, init, 0.4, drop=e >= (n // 128) * 128)[0], ref, bound, 'the last 128-element chunk dropped')
    rejects(R.pairmin(x, 1, 3, 1, mask, init, 0.4, drop=e >= 4096 * 128)[0], ref, bound, 'the second grid-stride chunk dropped')
    g, tie = R.pairmin_grad(x, 1, 3, 1, mask, init, 0.4, -0.7)
    gb = 4 * U * g.abs() + 1e-300
    gb[:, tie] = float('inf')
    assert R.compare(r32(g), g, gb) <= 1
    rejects(R.pairmin_grad(x, 1, 3, 1, mask, init, 0.4, -0.7, highest_on_tie=True)[0], g, gb, 'the highest index on an exact tie')
    x4, _, _ = G.pair_case('tie3')
    g4, t4 = R.pairmin_grad(x4, 0, 4, 1, None, None, 0.4, -0.7)
    b4 = 4 * U * g4.abs() + 1e-300
    b4[:, t4] = float('inf')
    rejects(R.pairmin_grad(x4, 0, 4, 1, None, None, 0.4, -0.7, highest_on_tie=True)[0], g4, b4, 'the highest index on an exact tie')
    rejects(g4 * ((x4 > 0) & (x4 < 1)), g4, b4, 'exclusive gate')


def test_planted_kde():
    X, bins = G.kde_case(49)
    ranges = [(0, 128), (128, 257)]
    ref = R.kde_fwd(X, bins, ranges, 1.0, 5e-3)
    bound = R.rtol_bound(ref, 1e-5)
    assert R.compare(ref + 0.5e-5 * ref, ref, bound) <= 1
    rejects(R.kde_fwd(X, bins, ranges, 1.0, 5e-3, skip_d=48), ref, bound, 'one d of a D = 49 point skipped')
    rejects(R.kde_fwd(X, bins, [(0, 128), (128, 256)], 1.0, 5e-3), ref, bound, 'the point after two LDS chunks dropped')
    rejects(R.kde_fwd(X, bins, ranges, 2.0, 5e-3), ref, bound, 'no wrap at |delta| > 1')
    # the older helpers agree with the ABI-level forms
    lse, grad = R._ref_rows(X, bins, 5e-3, torch.ones(X.size(0), dtype=torch.float64))
    np.testing.assert_allclose(lse.numpy(), torch.logsumexp(ref, 0).numpy(), rtol=1e-12)
    mine = R.kde_bwd(X, [(0, 0, 256), (0, 256, 300)], bins, 1.0, 5e-3, l_row=lse)
    np.testing.assert_allclose(mine.numpy(), grad.numpy(), rtol=1e-9, atol=1e-12)
    tiles = [(0, 0, 250), (0, 256, 299), (1, 299, 300)]
    gr = R.kde_bwd(X, tiles, bins, 1.0, 5e-3, l_row=lse.float())
    live = torch.isfinite(gr[:, 0])
    assert int((~live).sum()) == 6                              # rows 250 .. 255 lie in no tile
    gb = R.rtol_bound(gr[live], 2e-3, 1e-5)
    rejects(R.kde_bwd(X, tiles, bins[:200], 1.0, 5e-3, l_row=lse.float())[live], gr[live], gb, 'the ragged last slab of bins dropped')
    rejects(R.kde_bwd(X, tiles, bins, 1.0, 5e-3)[live], gr[live], gb, 'l_row ignored')
    b, hw = G.dedup_case(4)
    keep = R.kde_dedup(b, hw)
    assert not G.same_bits(keep, R.kde_dedup(b.flip(0), hw).flip(0)), 'the earlier bin dropped in place of the later one goes unnoticed'
    assert keep[255] == 0 and keep[10] == 0 and keep[127] == 0 and keep[256] == 1 and keep[3] == 1


# =================================================================================================== the tie caps, by the reference alone
def test_tie_caps_of_the_gpu_cases():
    for Cc in (1, 3):
        for nx in (257, 290):
            for ny in (1, 7):
                for fr in (False, True):
                    x, mask, bx, fx, by, fy, g = G.shift_case(Cc, nx, ny, fr)
                    tie = R.shift_l1_grad(x, mask, bx, fx, by, fy, g)[3]
                    assert float(tie.double().mean()) <= R.TIE_CAP, (Cc, nx, ny, fr)
                    assert bool((x == 0).any()) and bool((x == 1).any())
    for name, c in G.PAIR_CASES.items():
        x, mask, init = G.pair_case(name)
        tie = R.pairmin_grad(x, c[4], c[5], c[6], mask, init, 0.4, -0.7)[1]
        assert float(tie.double().mean()) <= R.PAIRMIN_TIE_CAP, name


# =================================================================================================== refusals
def _dev():
    return 'cuda' if torch.cuda.is_available() else 'cpu'


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream) if torch.cuda.is_available() else None


class Out:
    """an output buffer: NaN (float) or 0xA5 (integer) before every call"""

    def __init__(self, n, dtype=torch.float32):
        self.t = torch.empty(int(n), dtype=dtype, device=_dev())
        self.fill()

    def fill(self):
        if self.t.dtype.is_floating_point:
            self.t.fill_(float('nan'))
        else:
            self.t.view(torch.uint8).fill_(0xA5)

    def untouched(self):
        return bool(torch.isnan(self.t).all()) if self.t.dtype.is_floating_point else bool((self.t.view(torch.uint8) == 0xA5).all())


def inp(n, dtype=torch.float32, value=0.5):
    return torch.full((int(n),), value, dtype=dtype, device=_dev())


def invoke(name, args, mut=None):
    L = G.lib()
    a = list(args)
    for k, v in (mut or {}).items():
        a[k] = v
    outs = [v for v in args if isinstance(v, Out)]
    for o in outs:
        o.fill()
    ptr = lambda v: v.t.data_ptr() if isinstance(v, Out) else (v.data_ptr() if torch.is_tensor(v) else v)  # noqa: E731
    rc = getattr(L, name)(*[ptr(v) for v in a], _stream())
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    if rc in (E_ARG, E_UNSUPPORTED):
        assert all(o.untouched() for o in outs), '%s: a refused call wrote to an output' % name
    return rc


def refusal_cases():
    f, i32, u8, f64 = torch.float32, torch.int32, torch.uint8, torch.float64
    cs = []

    def add(name, args, muts):
        cs.append((name, args, muts))
    # esr_soft_hist_*: (v, n, K, lo, hi, T, eps, ...); the buffers hold 4097 bins
    hist = [inp(100), 100, 64, 0.0, 1.0, 2e-3, 1e-7]
    hm = [('null_v', {0: None}), ('n_0', {1: 0}), ('K_0', {2: 0}), ('K_4097', {2: 4097}), ('T_0', {5: 0.0}), ('hi_eq_lo', {4: 0.0}), ('hi_below_lo', {3: 2.0})]
    add('esr_soft_hist_fwd', hist + [Out(4097, f64)], hm + [('null_partial', {7: None})])
    add('esr_soft_hist_bwd', hist + [inp(4097), Out(100)], hm + [('null_gh', {7: None}), ('null_gv', {8: None})])
    # esr_kde_*: two outer points; the range and slab tables hold 65536 entries for the grid-limit cases
    rng_ = torch.zeros(2 * 65536, dtype=i32, device=_dev())
    rng_[1::2] = 3
    add('esr_kde_fwd', [inp(2 * 4), 2, inp(3 * 4), rng_, 2, 4, 1.0, 50.0, Out(2 * 65536), Out(2 * 65536, f64)],
        [('null_outer', {0: None}), ('null_inner', {2: None}), ('null_ranges', {3: None}), ('null_pmax', {8: None}), ('null_psum', {9: None}),
         ('n_outer_0', {1: 0}), ('n_ranges_0', {4: 0}), ('n_ranges_65536', {4: 65536}), ('D_10', {5: 10}), ('D_0', {5: 0}), ('scale_0', {7: 0.0})])
    tiles = torch.tensor([0, 0, 2], dtype=i32, device=_dev())
    add('esr_kde_bwd', [inp(2 * 4), 2, tiles, 1, inp(5 * 4), 5, 3, 2, 4, 1.0, 50.0, inp(2), inp(2), inp(5), inp(5), Out(65536 * 2 * 4)],
        [('null_X', {0: None}), ('null_tiles', {2: None}), ('null_bins', {4: None}), ('null_dxpart', {15: None}), ('R_0', {1: 0}), ('n_tiles_0', {3: 0}),
         ('M_0', {5: 0}), ('bins_per_slab_0', {6: 0}), ('n_slabs_0', {7: 0}), ('n_slabs_65536', {7: 65536}), ('slabs_short_of_M', {6: 2}),
         ('D_10', {8: 10}), ('scale_0', {10: 0.0}), ('g_bin_without_l_bin', {14: None}), ('l_bin_without_g_bin', {13: None})])
    add('esr_kde_dedup', [inp(5 * 4), 5, 4, 0.01, Out(5, i32)], [('null_bins', {0: None}), ('null_keep', {4: None}), ('M_0', {1: 0}), ('D_10', {2: 10})])
    # esr_img_stats*: (x, B, C, H, W, mask, clamp01, kind, ...)
    img = [inp(2 * 3 * 8 * 9), 2, 3, 8, 9, inp(72), 1]
    dims = [('B_0', {1: 0}), ('C_0', {2: 0}), ('H_0', {3: 0}), ('W_0', {4: 0})]
    add('esr_img_stats', img + [2, Out(6, f64)], [('null_x', {0: None}), ('null_sums', {8: None}), ('kind_-1', {7: -1}), ('kind_3', {7: 3})] + dims)
    add('esr_img_stats_grad', img + [2, inp(6), Out(432), 0],
        [('null_x', {0: None}), ('null_coef', {8: None}), ('null_dx', {9: None}), ('kind_-1', {7: -1}), ('kind_3', {7: 3})] + dims)
    # the patch kernels: 65536 images of 1 x 7 x 7 for the grid limit
    NB = 65536
    px, small = inp(NB * 49), [('H_6', {3: 6}), ('W_6', {4: 6}), ('B_65536', {1: NB}, E_UNSUPPORTED)]
    add('esr_patch_std', [px, 2, 1, 7, 7, inp(1, u8, 1), Out(NB), Out(NB)],
        [('null_x', {0: None}), ('null_corners', {5: None}), ('null_S', {6: None}), ('null_mean', {7: None})] + dims[:2] + small)
    add('esr_patch_std_grad', [px, 2, 1, 7, 7, inp(1, u8, 1), inp(NB), inp(NB), inp(NB), Out(NB * 49), 0],
        [('null_x', {0: None}), ('null_corners', {5: None}), ('null_S', {6: None}), ('null_mean', {7: None}), ('null_dS', {8: None}),
         ('null_dx', {9: None})] + dims[:2] + small)
    ci = torch.zeros(1, dtype=i32, device=_dev())
    add('esr_patch_mag', [px, 2, 1, 7, 7, ci, inp(49), 1, Out(NB, f64)],
        [('null_x', {0: None}), ('null_index', {5: None}), ('null_desired', {6: None}), ('null_partial', {8: None}), ('P_0', {7: 0})] + dims[:2] + small)
    add('esr_patch_mag_grad', [px, 2, 1, 7, 7, ci, inp(49), 1, inp(NB), Out(NB * 49), 0],
        [('null_x', {0: None}), ('null_index', {5: None}), ('null_desired', {6: None}), ('null_g', {8: None}), ('null_dx', {9: None}), ('P_0', {7: 0})]
        + dims[:2] + small)
    # esr_shift_l1*: (x, B, C, H, W, mask, nx, ny, base_x, frac_x, base_y, frac_y, ...): 1 x 1 images, one output column, up to 65536 rows / images
    zi = torch.zeros(2 * NB, dtype=i32, device=_dev())
    sh = [inp(NB), 2, 1, 1, 1, inp(1), 1, 2, zi, inp(2 * NB, value=0.25), zi, inp(2 * NB, value=0.25)]
    sm = [('null_x', {0: None}), ('null_mask', {5: None}), ('null_base_x', {8: None}), ('null_frac_x', {9: None}), ('null_base_y', {10: None}),
          ('null_frac_y', {11: None}), ('nx_0', {6: 0}), ('ny_0', {7: 0}), ('B_65536', {1: NB}, E_UNSUPPORTED)] + dims
    add('esr_shift_l1', sh + [Out(NB * 2, f64)], sm + [('null_partial', {12: None})])
    rr = torch.zeros(4, dtype=i32, device=_dev())
    add('esr_shift_l1_grad', sh + [rr, rr, inp(NB), Out(2 * NB), Out(NB), 0],
        sm + [('null_ranges_x', {12: None}), ('null_ranges_y', {13: None}), ('null_g', {14: None}), ('null_work', {15: None}), ('null_dx', {16: None}),
              ('ny_65536', {7: NB}, E_UNSUPPORTED)])
    # esr_scribble*: (x, B, C, H, W, desired, labels, i0, i0_batch, ...): 1 x 1 images
    sc = [inp(NB), 3, 1, 1, 1, inp(1), inp(1, u8, 0xC1), inp(3), 3]
    scm = [('null_x', {0: None}), ('null_desired', {5: None}), ('null_labels', {6: None}), ('i0_batch_2_of_3', {8: 2}), ('i0_batch_0', {8: 0}),
           ('B_65536', {1: NB, 8: 1}, E_UNSUPPORTED)] + dims
    add('esr_scribble', sc + [Out(NB * 5, f64)], scm + [('null_partial', {9: None})])
    add('esr_scribble_grad', sc + [inp(NB), 0.35, Out(NB), 0], scm + [('null_g', {9: None}), ('null_dx', {11: None})])
    # esr_pairmin*: (x, Bg, C, H, W, lo, hi, clamp01, mask, init, init_batch, w, ...): 10241 rows of one element
    NR = 10241
    pm = [inp(NR), 4, 1, 1, 1, 1, 4, 1, inp(1), inp(NR), 3, 0.4]
    pmm = [('null_x', {0: None}), ('Bg_0', {1: 0}), ('C_0', {2: 0}), ('H_0', {3: 0}), ('W_0', {4: 0}), ('lo_-1', {5: -1}), ('hi_eq_lo', {6: 1}),
           ('hi_above_Bg', {6: 5}), ('init_batch_2_of_3', {10: 2}), ('init_batch_4_of_3', {10: 4})]
    add('esr_pairmin', pm + [inp(NR), Out(NR, f64)], pmm + [('null_partial', {13: None}), ('work_null_beyond_lds', {1: 400, 6: 4, 12: None}),
                                                           ('rows_beyond_lds', {1: NR, 5: 0, 6: NR, 10: 1}, E_UNSUPPORTED)])
    add('esr_pairmin_grad', pm + [-0.7, inp(NR), Out(NR)], pmm + [('null_dx', {14: None}), ('work_null_beyond_lds', {1: 400, 6: 4, 13: None})])
    return cs


_CASES = None


def _cases():
    global _CASES
    if _CASES is None:
        _CASES = {c[0]: c for c in refusal_cases()}
    return _CASES


ENTRY_POINTS = ['esr_soft_hist_fwd', 'esr_soft_hist_bwd', 'esr_kde_fwd', 'esr_kde_bwd', 'esr_kde_dedup', 'esr_img_stats', 'esr_img_stats_grad',
                'esr_patch_std', 'esr_patch_std_grad', 'esr_patch_mag', 'esr_patch_mag_grad', 'esr_shift_l1', 'esr_shift_l1_grad', 'esr_scribble',
                'esr_scribble_grad', 'esr_pairmin', 'esr_pairmin_grad']


@pytest.mark.parametrize('name', ENTRY_POINTS)
def test_refused(name):
    _, args, muts = _cases()[name]
    assert invoke(name, args) not in (E_ARG, E_UNSUPPORTED), 'the unmodified call is refused'
    for m in muts:
        tag, mut, want = m if len(m) == 3 else (m + (E_ARG,))
        assert invoke(name, args, mut) == want, '%s %s' % (name, tag)
    # NULL optional pointers are no reason to refuse
    if name.startswith('esr_scribble'):
        assert invoke(name, args, {7: None, 8: 2}) not in (E_ARG, E_UNSUPPORTED), 'i0 NULL: i0_batch is not looked at'
    if name.startswith('esr_pairmin'):
        assert invoke(name, args, {8: None, 9: None, 10: 7}) not in (E_ARG, E_UNSUPPORTED), 'init NULL: init_batch is not looked at'
    if name.startswith('esr_img_stats'):
        assert invoke(name, args, {5: None}) not in (E_ARG, E_UNSUPPORTED)


def test_size_queries():
    L = G.lib()
    assert L.esr_soft_hist_slabs(0) == E_ARG and L.esr_soft_hist_slabs(4096) == 1 and L.esr_soft_hist_slabs(4097) == 2
    assert [L.esr_kde_dim_supported(d) for d in (0, 1, 2, 4, 9, 10, 16, 25, 36, 49, 64, 81)] == [0, 1, 0, 1, 1, 0, 1, 1, 1, 1, 1, 0]
    assert L.esr_patch_mag_blocks(6, 7) == 0 and L.esr_patch_mag_blocks(7, 7) == 1 and L.esr_patch_mag_blocks(23, 71) == 4
    assert L.esr_pairmin_blocks(0, 1, 1) == E_ARG and L.esr_pairmin_blocks(1, 513, 1023) == 4096 and L.esr_pairmin_blocks(1, 1, 129) == 2
    assert L.esr_pairmin_work_floats(3, 1, 1, 1, 2, 2, 0) == E_ARG and L.esr_pairmin_work_floats(3, 1, 1, 1, 0, 4, 1) == E_ARG
    assert L.esr_pairmin_work_floats(161, 1, 3, 50, 0, 161, 0) == 0 and L.esr_pairmin_work_floats(161, 1, 3, 50, 0, 161, 1) == 161 * 150
    assert L.esr_pairmin_work_floats(160, 1, 3, 50, 0, 160, 1) == 0

"""CPU tests of the local-STD and periodicity Z objectives' host side (esr_hip/local.py; reference codes/Z_optimization.py:391-398, 459-509,
616-627, 799-815): the corner map and the coordinate lines against what the reference built (fixture tests/golden/local_z.npz, written by
tools/gen_local_z_golden.py), the CPU paths of the losses and their gradients against the reference's values, the C-ABI's argument checks,
and the refusals of what this build does not implement."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'local_z.npz')
CASES = ('nonint1', 'nonint2', 'int1')


def golden():
    return np.load(GOLDEN)


def test_corner_map_is_the_references_patch_set():
    from esr_hip import local
    g = golden()
    mask = g['a/mask']
    corners = local.patch_corners(mask)
    assert corners.dtype == np.uint8 and corners.shape == (mask.shape[0] - 6, mask.shape[1] - 6)
    np.testing.assert_array_equal(local.corner_patch_indexes(corners, mask.shape[1]), g['a/patches'])


def test_corner_map_without_mask_is_every_window_and_an_empty_region_raises():
    from esr_hip import local
    c = local.patch_corners(None, 20, 17)
    assert c.shape == (14, 11) and c.all()
    m = np.zeros((20, 17), np.float32)
    m[2:8, 3:15] = 1                                         # 6 rows: no 7 x 7 window
    with pytest.raises(ValueError, match='no 7 x 7 patch'):
        local.patch_corners(m)


@pytest.mark.parametrize('case', ['nonint1', 'nonint2'])
def test_coordinate_lines_equal_the_references_grids(case):
    from esr_hip import local
    g = golden()
    H, W = g['a/mask'].shape
    for k, point in enumerate(g['a/%s/points' % case]):
        for s, (xl, yl) in enumerate(local.periodicity_lines(point, H, W)):
            np.testing.assert_array_equal(xl, g['a/%s/lines%d_%d_x' % (case, k, s)])
            np.testing.assert_array_equal(yl, g['a/%s/lines%d_%d_y' % (case, k, s)])


def test_cpu_patch_std_and_gradient_match_the_reference():
    from esr_hip import local
    g = golden()
    x = torch.from_numpy(g['a/x']).requires_grad_(True)
    ps = local.PatchSet(g['a/mask'], *g['a/mask'].shape)
    S = local.patch_std(x, ps)
    np.testing.assert_allclose(S.detach().numpy(), g['a/std/S'], rtol=1e-5, atol=1e-7)
    (S * torch.from_numpy(g['a/std/cot'])).sum().backward()
    np.testing.assert_allclose(x.grad.numpy(), g['a/std/grad'], rtol=1e-5, atol=1e-5 * np.abs(g['a/std/grad']).max())


@pytest.mark.parametrize('case', CASES)
def test_cpu_periodicity_loss_and_gradient_match_the_reference(case):
    from esr_hip import local
    g = golden()
    mask = g['a/mask']
    H, W = mask.shape
    x = torch.from_numpy(g['a/x']).requires_grad_(True)
    ps = local.PatchSet(mask, H, W)
    pairs = [local.ShiftPair(p, H, W, interpolated='nonint' in case) for p in g['a/%s/points' % case]]
    S = local.patch_std(x, ps)
    initial = local.patch_std(x[:1].detach(), ps)
    np.testing.assert_allclose(initial.numpy(), g['a/%s/initial_STD' % case], rtol=1e-5, atol=1e-7)
    loss = (20 * (S - initial) ** 2).mean() + local.shift_l1(x, torch.from_numpy(mask), pairs)
    np.testing.assert_allclose(loss.detach().numpy(), g['a/%s/loss' % case], rtol=1e-5)
    loss.sum().backward()
    gr = g['a/%s/grad' % case]
    np.testing.assert_allclose(x.grad.numpy(), gr, rtol=1e-5, atol=1e-5 * np.abs(gr).max())


def test_flat_patch_has_zero_gradient_on_cpu():
    from esr_hip import local
    x = torch.full((1, 3, 9, 9), 0.4)
    x[:, :, :, 7:] = torch.linspace(0, 1, 18).view(1, 3, 3, 2).repeat(1, 1, 3, 1)
    x.requires_grad_(True)
    S = local.patch_std(x, local.PatchSet(None, 9, 9))
    assert float(S[0, 0]) == 0.0
    S.sum().backward()
    assert torch.isfinite(x.grad).all() and float(x.grad[..., 0].abs().max()) == 0.0        # column 0: only flat windows (cx = 0) cover it


def test_shift_pair_taps_and_ranges_cover_every_contributor():
    from esr_hip import local
    H, W = 23, 31
    for interp, point in ((True, (2.5, -3.25)), (True, (-1.75, 4.5)), (False, (3, -2))):
        pr = local.ShiftPair(point, H, W, interpolated=interp)
        for s in range(2):
            for base, rng, n_src in ((pr.base_x[s], pr.ranges_x[s], W), (pr.base_y[s], pr.ranges_y[s], H)):
                for q in range(n_src):
                    touching = np.flatnonzero((base == q) | (base + 1 == q))
                    lo, hi = rng[q]
                    assert all(lo <= j < hi for j in touching), (interp, s, q, touching, lo, hi)
        assert np.all((pr.frac_x >= 0) & (pr.frac_x < 1)) and np.all((pr.frac_y >= 0) & (pr.frac_y < 1))


def test_integer_form_refuses_non_integer_points():
    from esr_hip import local
    with pytest.raises(ValueError, match='integer'):
        local.ShiftPair((2.5, 1), 20, 20, interpolated=False)


def test_c_abi_rejects_null_and_empty_arguments_without_a_gpu():
    from esr_hip import _lib
    lib = _lib.load_library()
    p = C.c_void_p(16)                      # never dereferenced: the checks come first
    E = _lib.ESR_E_ARG
    assert lib.esr_patch_std(None, 1, 3, 16, 16, p, p, p, None) == E
    assert lib.esr_patch_std(p, 1, 3, 16, 16, None, p, p, None) == E
    assert lib.esr_patch_std(p, 0, 3, 16, 16, p, p, p, None) == E
    assert lib.esr_patch_std(p, 1, 3, 6, 16, p, p, p, None) == E              # smaller than one window
    assert lib.esr_patch_std_grad(p, 1, 3, 16, 16, p, p, p, None, p, 0, None) == E
    assert lib.esr_patch_std_grad(p, 1, 0, 16, 16, p, p, p, p, p, 0, None) == E
    assert lib.esr_shift_l1(p, 1, 3, 16, 16, None, 8, 8, p, p, p, p, p, None) == E
    assert lib.esr_shift_l1(p, 1, 3, 16, 16, p, 0, 8, p, p, p, p, p, None) == E
    assert lib.esr_shift_l1_grad(p, 1, 3, 16, 16, p, 8, 8, p, p, p, p, None, p, p, p, p, 0, None) == E
    assert lib.esr_shift_l1_grad(p, 1, 3, 16, 16, p, 8, 0, p, p, p, p, p, p, p, p, p, 0, None) == E


def test_new_objectives_are_listed():
    from Z_optimization import Z_optimizer
    for name in ('local_max_STD', 'local_min_STD', 'local_STD_increase', 'local_STD_decrease', 'local_STD_TV', 'local_STD_periodicity',
                 'local_STD_nonInt_periodicity', 'local_STD_periodicity_1D', 'local_STD_nonInt_periodicity_1D', 'periodicity', 'nonInt_periodicity'):
        assert name in Z_optimizer.SUPPORTED, name


@pytest.mark.parametrize('objective,match', [
    ('local_STD_nonInt_periodicity_Plus', "'Plus' variant"), ('local_STD_Mag_increase', "'Mag' variant"), ('local_TV', 'without STD'),
    ('local_hist', 'without STD'), ('scribble', 'not part of this build'), ('patchhist_localSTD', 'localSTD')])
def test_refusals_name_what_they_refuse(objective, match):
    from Z_optimization import Z_optimizer
    with pytest.raises(NotImplementedError, match=match):
        Z_optimizer(objective, [8, 8], model=None, Z_range=1, max_iters=1, initial_LR=0.1)


@pytest.mark.parametrize('objective', ['local_STD_increase', 'local_STD_TV', 'nonInt_periodicity'])
def test_training_mode_and_region_constraint_mode_are_refused(objective):
    from Z_optimization import Z_optimizer
    with pytest.raises(NotImplementedError, match='HR_unpadder'):
        Z_optimizer(objective, [8, 8], model=None, Z_range=1, max_iters=1, initial_LR=0.1, HR_unpadder=lambda t: t)
    m = np.ones((8, 8), np.float32)
    m[:2] = 0
    with pytest.raises(NotImplementedError, match='non_local_Z_optimization'):
        Z_optimizer(objective, [8, 8], model=None, Z_range=1, max_iters=1, initial_LR=0.1, image_mask=m, Z_mask=m, non_local_Z_optimization=True)

#!/usr/bin/env python
"""TEST INFRASTRUCTURE ONLY (CPU, build container): writes tests/golden/special_z.npz by running the REFERENCE's own Z_optimizer
(codes/Z_optimization.py:331-815) with the names the GUI's special-behaviour button sends, imported read-only through oracle/_refshim.  Run:
    python tools/gen_special_z_golden.py

cv2 is not installed here: Z_optimization.dilate is pinned to the restatement of tools/gen_scribble_golden.py, and `1 - bool_tensor` is
evaluated as the reference's torch did (its uint8_comparisons), both needed by the region constraint only.

(a) function level, on seeded images of 64 x 80 (non-square), B = 2, x spanning [-0.1, 1.1], an irregular image mask.  Z_optimizer is
    constructed on a stand-in model that holds ONE initial image (the reference's patch-magnitude construction takes batch 1 only), with a
    constant block inside the mask (patches at the 1/255 STD floor), STD_increment 0.03.  The patch-magnitude loss has no method of its own in
    the reference, so both groups are evaluated by its optimize() itself, one iteration on the stand-in model, whose output is x + 0 Z with x
    a leaf: the per-image losses are its latest_Z_loss_values and B x.grad is d sum_b loss_b / d x (float32, as computed).
  a/x [2, 3, 64, 80], a/x_init [1, 3, 64, 80], a/mask [64, 80]
  a/mag/{increase,decrease}/desired [49, P], patches [P, 49], loss [2], grad
  a/plus/{nonint1,nonint2,whole}/loss [2], grad, desired_STD, points      'local_STD_nonInt_periodicityPlus' (whole: 'nonInt_periodicityPlus')
(b) Z_optimizer(...).optimize() on the F7 model (oracle/gen_golden.py::gen_F7: RRDB-1, latent 3, LR 24 x 28 -> HR 96 x 112, B = 3, 4 iterations,
    Adam lr 0.1, the seeded LR and initial Z of tools/gen_local_z_golden.py), 'local_Mag_increase' and 'local_STD_nonInt_periodicityPlus', each
    with the all-ones mask pair ('full'), with that generator's irregular image mask and rectangular Z mask ('irr') and with those and
    non_local_Z_optimization on ('irr_nonlocal').  The model's output at construction comes from the Z of seed 921 - its first sample alone
    for the patch-magnitude runs (batch 1, see above).  The search starts from the same Z, except with the constraint on, where it starts
    from a second seeded Z (seed 922) so that the constraint's |out - initial| has no ties at 0.
  b/mask/{irr_image,irr_Z}, b/<objective>/<case>/loss, Z_mask, final_Z_sub (Z[:, :, ::8, ::8])
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from oracle import _refshim  # noqa: E402
from oracle.weights import fill_formula_weights, seeded_uniform  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
H, W, B = 64, 80, 2
INCREMENT = 0.03
POINTS = {'nonint1': [[2.5, 3.25]], 'nonint2': [[2.5, 3.25], [-1.75, 4.5]], 'whole': [[2.5, 3.25], [-1.75, 4.5]]}
OBJECTIVES = ('local_Mag_increase', 'local_STD_nonInt_periodicityPlus')
CASES = ('full', 'irr', 'irr_nonlocal')


def mask_a():
    m = (seeded_uniform((H, W), 1700).numpy() > 0.2).astype(np.float32)
    m[:8] = 0
    m[:, -8:] = 0
    m[12:56, 10:50] = 1
    m[30:60, 50:70] = 1
    m[25, 30] = m[40, 20] = m[45, 60] = 0            # holes: the opening removes their surroundings
    return m


def x_init_a():
    x = seeded_uniform((1, 3, H, W), 1702, -0.1, 1.1)
    x[:, :, 14:32, 12:36] = 0.4                      # a constant block inside the mask: flat patches
    return x


class _StandIn:
    """what Z_optimizer's constructor and its optimize() read of a model: the output is the leaf x (+ 0 Z, so that the latent has a gradient)"""

    def __init__(self, x):
        self.x = x
        self.fake_H = x
        self.num_latent_channels = 3
        self.netG = torch.nn.Linear(1, 1)

    def Output_Batch(self, within_0_1=False):
        return torch.clamp(self.fake_H, 0, 1) if within_0_1 else self.fake_H

    def GetLatent(self):
        return torch.zeros(1, 3, H, W)

    def feed_data(self, data, **kw):
        self.Z = data['Z']

    def test(self, **kw):
        self.fake_H = self.x + 0 * self.Z


def evaluate(zo, x0):
    """one iteration of the reference's optimize() on x0 -> (loss per image, d sum_b loss_b / d x)"""
    x = x0.clone().requires_grad_(True)
    zo.model.x = x
    zo.optimize()
    return np.array(zo.latest_Z_loss_values, dtype=np.float64), (x.grad * x0.size(0)).numpy()


def part_a(Z_optimizer, out):
    x0 = seeded_uniform((B, 3, H, W), 1701, -0.1, 1.1)
    x_init, mask = x_init_a(), mask_a()
    out['a/x'], out['a/x_init'], out['a/mask'] = x0.numpy(), x_init.numpy(), mask
    kw = dict(Z_size=[H, W], Z_range=1, max_iters=1, initial_LR=0.1, batch_size=B, image_mask=mask, Z_mask=np.ones((H, W), np.float32))
    quiet = contextlib.redirect_stdout(io.StringIO())
    for sign in ('increase', 'decrease'):
        with quiet:
            zo = Z_optimizer(objective='local_Mag_' + sign, model=_StandIn(x_init.clone()), data={'STD_increment': INCREMENT}, **kw)
            mat = zo.patch_extraction_map.coalesce()
            rows, cols = mat.indices().numpy()
            P = mat.size(0) // 49
            idx = np.zeros(mat.size(0), np.int64)
            idx[rows] = cols
            key = 'a/mag/%s/' % sign
            out[key + 'patches'] = idx.reshape(49, P).T.copy()
            out[key + 'desired'] = zo.desired_patches.detach().numpy().astype(np.float32)
            out[key + 'loss'], out[key + 'grad'] = evaluate(zo, x0)
        print(sign, P, out[key + 'loss'], float(np.abs(out[key + 'grad']).max()))
    for case, pts in POINTS.items():
        objective = 'nonInt_periodicityPlus' if case == 'whole' else 'local_STD_nonInt_periodicityPlus'
        with quiet:
            zo = Z_optimizer(objective=objective, model=_StandIn(x_init.clone()), data={'STD_increment': INCREMENT, 'periodicity_points': pts}, **kw)
            key = 'a/plus/%s/' % case
            out[key + 'points'] = np.array(pts, dtype=np.float64)
            out[key + 'desired_STD'] = zo.desired_STD.detach().double().numpy()
            out[key + 'loss'], out[key + 'grad'] = evaluate(zo, x0)
        print(case, out[key + 'desired_STD'].shape, out[key + 'loss'], float(np.abs(out[key + 'grad']).max()))


def part_b(Z_optimizer, out):
    from gen_local_z_golden import Z_POINTS, z_masks
    from gen_scribble_golden import uint8_comparisons
    from oracle.gen_golden import _ref_opt
    import models
    quiet = contextlib.redirect_stdout(io.StringIO())
    with quiet:
        m = models.create_model(_ref_opt(False))
    fill_formula_weights(m.netG, gain=0.5)
    lr = seeded_uniform((1, 3, 24, 28), 920)
    Bz = 3
    irr_im, irr_z = z_masks()
    out['b/mask/irr_image'], out['b/mask/irr_Z'] = irr_im, irr_z
    ones = np.ones([96, 112], dtype=np.float32)
    for obj in OBJECTIVES:
        for case in CASES:
            im_mask, z_mask = (ones, ones) if case == 'full' else (irr_im, irr_z)
            nonlocal_ = case == 'irr_nonlocal'
            z0 = seeded_uniform((Bz, 3, 96, 112), 921, -0.3, 0.3)
            z1 = seeded_uniform((Bz, 3, 96, 112), 922, -0.3, 0.3)
            n0 = 1 if 'Mag' in obj else Bz
            m.feed_data({'LR': lr.expand(n0, -1, -1, -1).clone(), 'Z': z0[:n0].clone()}, need_GT=False)
            m.test()
            data = {'LR': lr.expand(Bz, -1, -1, -1).clone(), 'STD_increment': INCREMENT, 'periodicity_points': Z_POINTS}
            with quiet, uint8_comparisons():
                zo = Z_optimizer(objective=obj, Z_size=[96, 112], model=m, Z_range=1, max_iters=4, data=data, initial_Z=(z1 if nonlocal_ else z0).clone(),
                                 initial_LR=0.1, batch_size=Bz, image_mask=im_mask.copy(), Z_mask=z_mask.copy(), non_local_Z_optimization=nonlocal_)
                assert bool(zo.non_local_Z_optimization) == nonlocal_
                z = zo.optimize()
            key = 'b/%s/%s/' % (obj, case)
            out[key + 'loss'] = np.array(zo.loss_values, dtype=np.float64)
            out[key + 'Z_mask'] = zo.Z_mask.numpy().astype(np.float32)
            out[key + 'final_Z_sub'] = z[:, :, ::8, ::8].numpy().copy()
            print(obj, case, zo.loss_values)


def main():
    _refshim.install()
    np.bool = bool                     # the reference's np.bool (removed from NumPy); set after SciPy has imported
    from gen_scribble_golden import dilate
    import Z_optimization
    Z_optimization.dilate = dilate
    out = {}
    part_a(Z_optimization.Z_optimizer, out)
    if '--part-a-only' not in sys.argv:
        part_b(Z_optimization.Z_optimizer, out)
    np.savez_compressed(os.path.join(GOLDEN, 'special_z.npz'), **out)


if __name__ == '__main__':
    main()
